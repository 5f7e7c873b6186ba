/*
 * hnh_dist.h — C ABI of the host layer (libhnh_host.so): the HnH operator surface as opaque handles.
 *
 * The host layer itself is C++ and mirrors the reference's classes by name (Distributed_Sparse,
 * Sparse15D_Dense_Shift, Sparse15D_Sparse_Shift, Sparse25D_Cannon_Dense, Sparse25D_Cannon_Sparse, SpmatLocal,
 * CSRLocal, StandardKernel, FlexibleGrid, BufferPair — headers under distributed_sddmm_amd/csrc/host/, see
 * INTEGRATION.md); C++ callers include those headers directly.  This C ABI exposes the same operations
 * to non-C++ callers (the Python tests and bench.py bind it with ctypes).  Each function cites the
 * reference member it forwards to (file:line under /root/reference).
 *
 * Conventions: int status return (0 == HNH_OK, codes of hnh_kernels.h); no exception crosses the ABI;
 * hnh_host_last_error() returns the calling thread's last message.  Handles are not thread-safe; every
 * call must be made by the thread that drives the handle's rank.  All calls of one operation are
 * collective over the ranks of the world, like the reference's MPI-based methods.
 */
#ifndef HNH_DIST_H
#define HNH_DIST_H

#include <stddef.h>
#include <stdint.h>

#include "hnh_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hnh_world hnh_world;               /* one rank of a process group (MPI_COMM_WORLD analogue) */
typedef struct hnh_thread_group hnh_thread_group; /* shared state of an in-process ("loopback") group       */
typedef struct hnh_spmat hnh_spmat;               /* SpmatLocal                                             */
typedef struct hnh_dist hnh_dist;                 /* Distributed_Sparse subclass + its StandardKernel       */
typedef struct hnh_dense hnh_dense;               /* DenseMatrix (device resident)                          */
typedef struct hnh_vec hnh_vec;                   /* VectorXd   (device resident)                          */

/* KernelMode (sparse_kernels.h:13) and MatMode (common.h:21) */
#define HNH_K_SDDMM_A 0
#define HNH_K_SPMM_A 1
#define HNH_K_SPMM_B 2
#define HNH_K_SDDMM_B 3
#define HNH_AMAT 0
#define HNH_BMAT 1

/* transport callbacks for hnh_world_create_callback (blocking; pointers are in the backend's memory space) */
#ifndef HNH_COMM_CALLBACKS_DEFINED
#define HNH_COMM_CALLBACKS_DEFINED
typedef struct hnh_comm_callbacks {
    void* user;
    int (*sendrecv)(void* user, const void* sendbuf, size_t sendbytes, int dst, void* recvbuf, size_t recvbytes, int src);
    int (*barrier)(void* user);
    int (*allgather)(void* user, const void* send, void* recv, size_t bytes_per_rank);
} hnh_comm_callbacks;
#endif

const char* hnh_host_last_error(void);

/* Selects the library implementing hnh_kernels.h.  NULL / "" = the product HIP library next to
 * libhnh_host.so.  The product never loads anything else; tests pass the path of the oracle test double. */
int hnh_backend_load(const char* path);
const char* hnh_host_backend_name(void);

/* ---- process groups (replace MPI_Init / MPI_COMM_WORLD; benchmark_dist.cpp:35-36) */
int hnh_world_create_single(int device, hnh_world** out);
int hnh_thread_group_create(int nranks, hnh_thread_group** out);
int hnh_thread_group_destroy(hnh_thread_group* g);
int hnh_world_create_thread(hnh_thread_group* g, int rank, int device, hnh_world** out);
int hnh_rccl_unique_id(void* id128_host);
int hnh_world_create_rccl(int rank, int nranks, int device, const void* id128_host, hnh_world** out);
/* One process per GPU of ONE node without RCCL: receivers pull out of their peers' mapped buffers (hnh_kernels.h, "ipc").
 * `session` = the same string on every rank of the job (it names the node-local shared-memory rendezvous). */
int hnh_world_create_ipc(int rank, int nranks, int device, const char* session, hnh_world** out);
int hnh_world_create_callback(int rank, int nranks, int device, const hnh_comm_callbacks* cb, hnh_world** out);
int hnh_world_destroy(hnh_world* w);
int hnh_world_rank(hnh_world* w);
int hnh_world_size(hnh_world* w);
int hnh_world_barrier(hnh_world* w);
int hnh_world_sync(hnh_world* w);                      /* drain compute + communication streams */
/* World::set_solo (an addition, a MEASUREMENT entry point; loopback transport only): solo replay — while on, the rank runs its own
 * side of every collective call alone (each receive = a device copy of what it would send, host collectives and barriers local), so
 * one rank's kernel sequence + the HBM side of its exchange can be timed with the GPU to itself.  Results of such calls are void. */
int hnh_world_set_solo(hnh_world* w, int on);
int hnh_world_set_timing_sync(hnh_world* w, int on);   /* perf counters synchronise first (reference-like attribution) */
void* hnh_world_stream(hnh_world* w, int stream);      /* raw hipStream_t */
hnh_ctx* hnh_world_ctx(hnh_world* w);                  /* the rank's kernel-level context */
/* FlexibleGrid(nr, nc, nh, adjacency) (FlexibleGrid.hpp:41-94): out9 = i, j, k, rankInRow, rankInCol, rankInFiber,
 * row size, col size, fiber size; *ok = result of the broadcast self test (FlexibleGrid.hpp:169-201). */
/* Transport self-test (collective): runs ONE communication primitive on `count` doubles with known contents and reports the
 * largest deviation from the expected values.  bench.py --gpus N runs every one of them under a watchdog before the timed
 * region, so a transport problem shows up as "rank r, primitive X" instead of a hang (no reference counterpart). */
enum {
    HNH_PREFLIGHT_RING = 0,                 /* relay step: send to ring rank +1, receive from -1 */
    HNH_PREFLIGHT_MESH = 1,                 /* n - 1 explicit-peer pairs in one group (mesh fetch) */
    HNH_PREFLIGHT_ALLGATHER = 2,            /* over a layer sub-communicator */
    HNH_PREFLIGHT_REDUCE_SCATTER = 3,
    HNH_PREFLIGHT_ALLREDUCE = 4,
    HNH_PREFLIGHT_VARIABLE = 5,             /* allgatherv + reduce_scatter_v, ragged counts */
    HNH_PREFLIGHT_ALLTOALLV = 6,            /* device all-to-all of the set-up pipeline */
    HNH_PREFLIGHT_ALLGATHER_WORLD = 7,      /* native RCCL collective on the world communicator */
    HNH_PREFLIGHT_REDUCE_SCATTER_WORLD = 8,
    HNH_PREFLIGHT_COUNT = 9
};
int hnh_world_preflight(hnh_world* w, int what, int64_t count, double* max_err);
/* running hash / number of the communicator splits so far: identical on every rank iff they split in the same order */
int hnh_world_split_signature(hnh_world* w, uint64_t* signature, int* count);
int hnh_world_grid_probe(hnh_world* w, int nr, int nc, int nh, int adjacency, int* out9, int* ok);
/* Where every rank of the world runs (collective; `out` takes hnh_world_size() records, the same on every rank): process id, device
 * ordinal and PCI bus id of the rank's GPU and — RCCL transport — what its communicator reports about itself (ncclCommCount,
 * ncclCommUserRank, ncclCommCuDevice; -1 for the other transports).  A job whose ranks report fewer distinct bus ids than ranks shares
 * GPUs: bench.py prints these records so that its N > 1 line certifies where it ran (the reference's ranks are host processes). */
typedef struct hnh_rank_identity {
    int32_t rank, pid, device_ordinal;
    int32_t comm_count, comm_rank, comm_device;
    char pci_bus_id[40];
} hnh_rank_identity;
int hnh_world_identities(hnh_world* w, hnh_rank_identity* out);

/* ---- sparse input (SpmatLocal.hpp:267-606) */
/* Wraps tuples that this rank holds initially (any distribution; coords / M / N / dist_nnz as the reference's
 * drivers fill them).  Host arrays, copied. */
int hnh_spmat_create(hnh_world* w, int64_t M, int64_t N, int64_t dist_nnz, int64_t local_nnz, const int64_t* rows,
                     const int64_t* cols, const double* values, hnh_spmat** out);
/* SpmatLocal::loadTuples(readFromFile, logM, nnz_per_row, filename) (SpmatLocal.hpp:467-533) */
int hnh_spmat_load_tuples(hnh_world* w, int read_from_file, int logM, int nnz_per_row, const char* filename, hnh_spmat** out);
int hnh_spmat_info(hnh_spmat* s, int64_t out4[4]); /* M, N, dist_nnz, local tuple count */
/* seeded random relabelling of rows/columns for load balance (random_permute.cpp; twin: oracle.vertex_permutation) */
int hnh_spmat_permute(hnh_spmat* s, uint64_t seed);
int hnh_spmat_destroy(hnh_spmat* s);
/* the shared synthetic generator (bit-identical to oracle/oracle.py:erdos_renyi_mn) */
int hnh_er_generate(uint64_t m, uint64_t n, uint64_t draws, uint64_t seed, void** handle, int64_t* count);
/* skewed R-MAT stand-in for real graphs (initiator a, b, c, 1-a-b-c; twin: oracle/oracle.py:rmat) */
int hnh_rmat_generate(int logm, uint64_t edges, double a, double b, double c, uint64_t seed, int scramble, void** handle,
                      int64_t* count);
int hnh_er_fetch(void* handle, int64_t* rows, int64_t* cols); /* also frees the handle */
/* (an addition) writes the entries as a MatrixMarket coordinate file (1-based; values NULL = all 1; symmetric != 0: the header says so
 * and the caller passes one triangle), formatted by all host cores — the files the input side (loadTuples(readFromFile = true),
 * SpmatLocal.hpp:485-498) is tested and benchmarked with. */
int hnh_write_matrix_market(const char* path, int64_t M, int64_t N, int64_t n, const int64_t* rows, const int64_t* cols, const double* values,
                            int symmetric);

/* ---- operator construction (benchmark_dist.cpp:45-82): alg in
 *   "15d_fusion1" | "15d_fusion2" | "15d_sparse" | "25d_dense_replicate" | "25d_sparse_replicate" */
int hnh_dist_create(hnh_world* w, const char* alg, hnh_spmat* s, int R, int c, hnh_dist** out);
int hnh_dist_destroy(hnh_dist* d);
/* out16 = M, N, R, p, c, localArows, localAcols, localBrows, localBcols, len(like_S_values), len(like_ST_values),
 *         r_split, dist_nnz, proc_rank, #aSubmatrices, #bSubmatrices   (distributed_sparse.h:34-76) */
int hnh_dist_info(hnh_dist* d, int64_t out16[16]);
/* a/bSubmatrices (distributed_sparse.h:56-57): 4 ints each (topRow, leftCol, rowCount, colCount) */
int hnh_dist_submatrices(hnh_dist* d, int matmode, int64_t* out, int capacity_entries);
int hnh_dist_set_r(hnh_dist* d, int R); /* setRValue */
/* which: 0 = json_algorithm_info (distributed_sparse.h:131-179), 1 = json_perf_statistics (:245-261) */
int hnh_dist_json(hnh_dist* d, int which, char* buf, size_t capacity);
int hnh_dist_reset_timers(hnh_dist* d); /* reset_performance_timers */
/* HIP-event time of the local kernels launched by the operator's StandardKernel since enabling */
int hnh_dist_kernel_profile(hnh_dist* d, int enable, double* total_ms, int64_t* launches);
/* Borrowed value arrays of stationary blocks (an addition; HNH_BORROW=off|force, default = where it pays): block-level counts since
 * construction, S and ST together: [0] SpMM value arrays read in place from the caller's vector, [1] copied as setCSRValues does
 * (SpmatLocal.hpp:571-579), [2] SDDMM results written as SValues .* dots by the kernel, [3] by the closing Hadamard pass
 * (15D_dense_shift.hpp:366) */
int hnh_dist_borrow_stats(hnh_dist* d, int64_t out4[4]);

/* ---- dense operands / value vectors (device resident) */
int hnh_dense_create(hnh_world* w, int64_t rows, int64_t cols, double fill, hnh_dense** out);
int hnh_dense_wrap(hnh_world* w, void* device_ptr, int64_t rows, int64_t cols, hnh_dense** out); /* non-owning */
int hnh_dense_like(hnh_dist* d, int matmode, double fill, hnh_dense** out); /* like_A_matrix / like_B_matrix (:197-203) */
int hnh_dense_shape(hnh_dense* m, int64_t out2[2]);
void* hnh_dense_data(hnh_dense* m); /* device pointer; may change after an operation that hands storage back */
int hnh_dense_upload(hnh_dense* m, const double* host);
int hnh_dense_download(hnh_dense* m, double* host);
int hnh_dense_fill(hnh_dense* m, double value);
int hnh_dense_copy(hnh_dense* dst, hnh_dense* src);
int hnh_dense_destroy(hnh_dense* m);
int hnh_dense_dummy_initialize(hnh_dist* d, hnh_dense* m, int matmode); /* dummyInitialize (:322-346) */
int hnh_vec_create(hnh_world* w, int64_t n, double fill, hnh_vec** out);
int hnh_vec_like(hnh_dist* d, int which /* 0 = like_S_values, 1 = like_ST_values (:189-195) */, double fill, hnh_vec** out);
int64_t hnh_vec_size(hnh_vec* v);
void* hnh_vec_data(hnh_vec* v);
int hnh_vec_upload(hnh_vec* v, const double* host);
int hnh_vec_download(hnh_vec* v, double* host);
int hnh_vec_fill(hnh_vec* v, double value);
int hnh_vec_destroy(hnh_vec* v);

/* ---- operations (distributed_sparse.h:268-320) */
int hnh_dist_initial_shift(hnh_dist* d, hnh_dense* A, hnh_dense* B, int kernel_mode);
int hnh_dist_de_shift(hnh_dist* d, hnh_dense* A, hnh_dense* B, int kernel_mode);
int hnh_dist_sddmmA(hnh_dist* d, hnh_dense* A, hnh_dense* B, hnh_vec* S, hnh_vec* result);
int hnh_dist_sddmmB(hnh_dist* d, hnh_dense* A, hnh_dense* B, hnh_vec* S, hnh_vec* result);
int hnh_dist_spmmA(hnh_dist* d, hnh_dense* A, hnh_dense* B, hnh_vec* S);
int hnh_dist_spmmB(hnh_dist* d, hnh_dense* A, hnh_dense* B, hnh_vec* S);
int hnh_dist_fusedSpMM(hnh_dist* d, hnh_dense* A, hnh_dense* B, hnh_vec* S, hnh_vec* sddmm_buffer, int matmode);
/* Distributed_Sparse::hold_moving_operand / release_moving_operand (an addition): a promise that the CONTENTS of `m` stay
 * the same until released (m = NULL), so a schedule may keep the blocks of it that it fetched from other ranks (the fixed
 * factor of an ALS half-step, als_conjugate_gradients.cpp:38-141).  Ignored by schedules that cannot use it. */
int hnh_dist_hold_moving_operand(hnh_dist* d, hnh_dense* m_or_null);
/* Distributed_Sparse::walk_windows_when_held (an addition, a MEASUREMENT entry point): with a held operand's blocks resident a call
 * runs one pass over them; on = 1 makes it walk the chunk windows as a fetching call does (own block, then windowed passes over what
 * has landed — everything, here), on = 2 one windowed pass per chunk (the sequence of a call whose chunks arrive one by one), so that
 * one rank's kernel sequence of a p-rank job can be timed alone on a GPU.  Same results either way. */
int hnh_dist_walk_windows_when_held(hnh_dist* d, int on);
/* Distributed_Sparse::fusedSpMM_out (an addition): out-of-place fusedSpMM with the applications' surrounding work in the
 * same pass — LeakyReLU between the halves (gat.hpp:96-99), Out += x_scale * X and rowdot[i] = <X[i,:], Out[i,:]>
 * (als_conjugate_gradients.cpp:93,282,295).  *supported = 0 and nothing done when the schedule has no single fused pass. */
int hnh_dist_fusedSpMM_out(hnh_dist* d, hnh_dense* A, hnh_dense* B, int matmode, hnh_dense* Out, int leaky, double leaky_alpha,
                           double x_scale, hnh_vec* rowdot_or_null, int* supported);
int hnh_dist_algorithm(hnh_dist* d, hnh_dense* A, hnh_dense* B, hnh_vec* S, hnh_vec* result_or_null, int kernel_mode,
                       int initial_replicate);

/* ---- ALS by batched conjugate gradients around fusedSpMM (als_conjugate_gradients.{h,cpp}; BASELINE config 5) */
typedef struct hnh_als hnh_als; /* Distributed_ALS */
/* Distributed_ALS(d_ops, artificial_groundtruth) (.cpp:148-184); random fills are hashes of global coordinates */
int hnh_als_create(hnh_dist* d, int artificial_groundtruth, uint64_t seed, hnh_als** out);
int hnh_als_destroy(hnh_als* a);
int hnh_als_set_ground_truth(hnh_als* a, hnh_vec* gt_S_order, hnh_vec* gt_ST_order); /* members ground_truth{,_transpose} */
int hnh_als_initialize_embeddings(hnh_als* a);                                         /* initializeEmbeddings (.cpp:221-233) */
int hnh_als_set_embeddings(hnh_als* a, hnh_dense* A, hnh_dense* B);                   /* members A, B (copied in)   */
int hnh_als_get_embeddings(hnh_als* a, hnh_dense* A, hnh_dense* B);                   /* members A, B (copied out)  */
int hnh_als_cg_optimizer(hnh_als* a, int matmode, int cg_max_iter);                    /* cg_optimizer (.cpp:38-141) */
int hnh_als_run_cg(hnh_als* a, int n_alternating_steps);                               /* run_cg (.cpp:235-263)      */
int hnh_als_compute_residual(hnh_als* a, double* out);                                 /* computeResidual (.cpp:201-219) */

/* ---- implicit-feedback ALS with confidence weights (an addition; csrc/host/als_implicit.hpp: Implicit_ALS).  The model of Hu, Koren and
 * Volinsky: preference 1 with confidence 1 + w_e on the stored pairs, preference 0 with confidence 1 on every other pair, every row
 * solved by a few guarded CG iterations.  Schedule 15d_fusion2 only (anything else is refused by name), lambda > 0.  Kernels: the Gram
 * matrices need include/hnh_grad.h; folded mode needs include/hnh_als_implicit.h (both optional groups: a kernel library without one
 * makes hnh_ials_half_step / _run / _loss / _gram fail with an error naming the missing symbol). */
typedef struct hnh_ials hnh_ials; /* Implicit_ALS */
int hnh_ials_create(hnh_dist* d, double lambda, uint64_t seed, hnh_ials** out);
int hnh_ials_destroy(hnh_ials* a);
/* w >= 0 and finite per stored pair, in the like_S_values and the like_ST_values layouts (copied in) */
int hnh_ials_set_confidence(hnh_ials* a, hnh_vec* w_S_order, hnh_vec* w_ST_order);
int hnh_ials_initialize_embeddings(hnh_ials* a);                      /* Distributed_ALS's hashed fill */
int hnh_ials_set_embeddings(hnh_ials* a, hnh_dense* A, hnh_dense* B); /* copied in  */
int hnh_ials_get_embeddings(hnh_ials* a, hnh_dense* A, hnh_dense* B); /* copied out */
int hnh_ials_half_step(hnh_ials* a, int matmode, int cg_iters);       /* the factor `matmode` names, the other one fixed */
int hnh_ials_run(hnh_ials* a, int n_alternating_steps, int cg_iters);
int hnh_ials_loss(hnh_ials* a, double* out);                          /* the objective, the same number on every rank */
int hnh_ials_gram(hnh_ials* a, int matmode, double* host_RxR);        /* A^T A or B^T B over all ranks, to host memory */
int hnh_ials_set_folded(hnh_ials* a, int folded);                     /* 1: hnh_gram_rows_f64 with the update; 0: the composed sequence */
/* The first k items (1 <= k <= 128) of each of the nq users (global row numbers, repeats allowed) by <a_u, b_j>, score descending and then
 * item id ascending: ids and scores are host arrays of nq x k, global item ids, the tail (-1, -infinity) where fewer than k items are
 * left.  filter_seen != 0: the items of the user's row of S are never returned.  Collective: every rank passes the same users and gets
 * the same result, bit-identical for every rank count.  Needs include/hnh_topk.h (an optional group; there is no host fallback). */
int hnh_ials_recommend(hnh_ials* a, const int64_t* users, int64_t nq, int k, int filter_seen, int64_t* ids, double* scores);
/* The exact position of items[i] in users[i]'s full ordering of all N items (the order of hnh_ials_recommend), for n pairs in global
 * coordinates, repeats allowed.  ranks[i]: the number of the user's candidates, other than items[i] itself, that rank before items[i],
 * 0-based; for an item the user has not seen it is the item's index in hnh_ials_recommend's list with k = infinity.  candidates[i]: N, or
 * with filter_seen != 0 (the items of the user's row of S are no candidates, the asked item always is) N - |seen_u \ {items[i]}|, so that
 * 0 <= ranks[i] < candidates[i].  in_seen (or NULL): 1 where filter_seen != 0 and items[i] is in the user's row of S, else 0.  Host
 * arrays of n int64.  Collective: every rank passes the same pairs and gets the same arrays, the same integers for every rank count.
 * Needs include/hnh_rank.h (an optional group; there is no host fallback) and R <= HNH_RANK_MAX_R. */
int hnh_ials_rank_of(hnh_ials* a, const int64_t* users, const int64_t* items, int64_t n, int filter_seen, int64_t* ranks, int64_t* candidates,
                     int64_t* in_seen);

/* ---- GAT forward pass (gat.hpp; BASELINE config 5's second application) */
typedef struct hnh_gat hnh_gat; /* GAT */
/* GAT(layers, d_ops) (gat.hpp:57-81): spec3 = {input_features, features_per_head, num_heads} per layer */
int hnh_gat_create(hnh_dist* d, int nlayers, const int* spec3, double leaky_relu_alpha, hnh_gat** out);
int hnh_gat_destroy(hnh_gat* g);
int hnh_gat_weight_shape(hnh_gat* g, int layer, int head, int64_t out2[2]);       /* layers[l].wMats[h] */
int hnh_gat_set_weight(hnh_gat* g, int layer, int head, const double* host);      /* row-major, host */
int hnh_gat_set_input(hnh_gat* g, hnh_dense* X);                                  /* buffers[0] (copied in)  */
int hnh_gat_get_output(hnh_gat* g, hnh_dense* out);                               /* buffers.back() (copied) */
int hnh_gat_buffer_shape(hnh_gat* g, int index, int64_t out2[2]);                 /* buffers[index]          */
int hnh_gat_forward(hnh_gat* g);                                                  /* forwardPass (gat.hpp:106-112) */
/* Backward pass (an addition: the reference's gat.hpp:43-48 leaves it as work in progress).  grad_out = dL/d(output) in the layout of
 * the last buffer.  Needs a forward pass since the last set_weight / set_input; 15d_fusion1 (any c) and 15d_fusion2 with c = 1 only
 * (HNH_ERR_INVALID otherwise, and when the kernel library lacks the kernels of include/hnh_grad.h). */
int hnh_gat_backward(hnh_gat* g, hnh_dense* grad_out);
int hnh_gat_get_weight_grad(hnh_gat* g, int layer, int head, double* host); /* dL/dW (hnh_gat_weight_shape), summed over all ranks */
int hnh_gat_get_input_grad(hnh_gat* g, hnh_dense* out);                     /* dL/d(buffers[0]) in its layout (copied)          */
/* Export of the attention coefficients (an addition; include/hnh_attn_coef.h).  out (hnh_vec_like's S layout: one entry per nonzero of S on
 * this rank) receives a_ij = exp(z_ij - lse_i) of (layer, head) of the STORED forward pass, in every score mode; with dropped != 0 and a
 * nonzero attention dropout rate c m_ij a_ij, the weights the aggregate used.  One pass over the nonzeros on the compute stream; the stored
 * pass, the gradients, the seed and the optimizer state are not touched, and the operator's R is what it was.  Attention SOFTMAX on 15d_fusion2
 * with c = 1, heads of at most 256 features; fails elsewhere before anything is launched, naming the argument, the mode (attention NONE: those
 * weights are what hnh_dist_sddmmA and hnh_leaky_relu_f64 give), the schedule, the width, the missing symbol, or the missing forward pass. */
int hnh_gat_attention_coefficients(hnh_gat* g, int layer, int head, int dropped, hnh_vec* out);
/* Attention mode (an addition).  NONE (the default of hnh_gat_create): the LeakyReLU scores are the edge weights, as in the
 * reference.  SOFTMAX: they are normalised over each row's neighbourhood, a_ij = exp(s_ij - lse_i), forward and backward; 15d_fusion2
 * with c = 1 only (the forward pass returns HNH_ERR_INVALID elsewhere, and when the kernel library lacks include/hnh_attention.h).
 * A change of mode invalidates the stored forward pass. */
#define HNH_GAT_ATTENTION_NONE 0
#define HNH_GAT_ATTENTION_SOFTMAX 1
int hnh_gat_set_attention(hnh_gat* g, int mode);
/* Backward mode (an addition).  UNFUSED (the default of hnh_gat_create): seven operator calls per head (4 SDDMM, 3 SpMM) with their
 * per-nonzero value vectors.  FUSED: the same gradients from two passes per head (include/hnh_attn_grad.h: one gather per layout);
 * 15d_fusion2 with c = 1 and heads of at most 256 features only — hnh_gat_backward fails elsewhere, naming the schedule or the
 * limit, or the missing symbol when the kernel library lacks the group.  An unknown mode fails; switching needs no new forward pass. */
#define HNH_GAT_BACKWARD_UNFUSED 0
#define HNH_GAT_BACKWARD_FUSED 1
int hnh_gat_set_backward(hnh_gat* g, int mode);
/* Score (an addition).  DOT (the default of hnh_gat_create): e_ij = LeakyReLU(<A_i, A_j>), everything above.  ADDITIVE: the two learned
 * vectors of a layer score an edge, e_ij = LeakyReLU(<A_i, a1_h> + <A_j, a2_h>) (include/hnh_attn_additive.h), forward and backward;
 * attention SOFTMAX on 15d_fusion2 with c = 1 and heads of at most 256 features only — hnh_gat_forward / hnh_gat_backward fail elsewhere,
 * naming the schedule, the mode or the width, or the missing symbol when the kernel library lacks the group.  With ADDITIVE there is one
 * backward implementation: the backward mode is not consulted.  A change of score invalidates the stored forward pass; an unknown one fails.
 * a1 / a2 (features_per_head doubles each, per layer and head) are zero until set; setting them invalidates the forward pass like
 * hnh_gat_set_weight.  Their gradients (summed over all ranks) are available after hnh_gat_backward with score ADDITIVE.
 * GATV2 (Brody, Alon, Yahav: dynamic attention): e_ij = sum_c a_hc LeakyReLU(A_ic + A_jc) with ONE learned vector per head, the nonlinearity
 * inside the contraction and none outside (include/hnh_attn_v2.h; shared weights: the same A scores and is aggregated), forward and backward;
 * attention SOFTMAX on 15d_fusion2 with c = 1, heads of at most 256 features and no attention dropout only, refused elsewhere like ADDITIVE, and
 * like it with one backward implementation.  The head's vector is a1 of hnh_gat_set_attn_vectors (a2 is kept and not used); after
 * hnh_gat_backward hnh_gat_get_attn_grads returns its gradient as da1 and zeros as da2.
 * TRANSFORMER (TransformerConv / UniMP: scaled dot-product attention with separate projections): s_ij = <Q_i, K_j> / sqrt(f) with Q = X W_q,
 * K = X W_k and the aggregate over V = X W_v, W_v being the head's weight of hnh_gat_set_weight (include/hnh_attn_qkv.h), forward and backward;
 * supported where GATV2 is and refused elsewhere like it, with one backward implementation; hnh_gat_attention_coefficients refuses it.  W_q and
 * W_k (hnh_gat_weight_shape each, per layer and head; which = 0: query, 1: key) are zero until set, which is a stationary point (uniform
 * attention, zero gradients of both): callers initialise them.  Setting one invalidates the forward pass; after hnh_gat_backward with this score
 * their gradients (summed over all ranks) can be read, and hnh_gat_optimizer_step updates them with the other parameters; hnh_gat_set_score
 * to another score drops them, and hnh_gat_get_qk_weight_grad refuses until the next hnh_gat_backward with this score. */
#define HNH_GAT_SCORE_DOT 0
#define HNH_GAT_SCORE_ADDITIVE 1
#define HNH_GAT_SCORE_GATV2 2
#define HNH_GAT_SCORE_TRANSFORMER 3
int hnh_gat_set_score(hnh_gat* g, int mode);
int hnh_gat_set_qk_weight(hnh_gat* g, int layer, int head, int which, const double* host);
int hnh_gat_get_qk_weight(hnh_gat* g, int layer, int head, int which, double* host);
int hnh_gat_get_qk_weight_grad(hnh_gat* g, int layer, int head, int which, double* host);
/* A per-edge bias on the logits of a layer with score TRANSFORMER (an addition; include/hnh_attn_edge.h): s_ij = <Q_i, K_j> / sqrt(f) + b_ij with
 * one finite value per nonzero of S on this rank, shared by the layer's heads and not learned (b = log w is the weighted neighbourhood softmax;
 * a distance or relation bias; -1e300 removes an edge from every row that keeps one of moderate bias; a row's largest bias should stay within
 * +-1e6, and a row of several edges ALL switched off is not supported: include/hnh_attn_edge.h; -inf is not supported).  It is given in both orders:
 * `s` in hnh_vec_like's S layout and `st` in its S^T layout (a probe SDDMM of row or column numbers names every entry's coordinates); the
 * caller keeps them in agreement, and two copies of a repeated pair may carry different values.  Both are copied; both NULL clears the bias and the
 * layer launches what it launched before.  One NULL, a wrong length or a layer out of range is refused and leaves the object as it was.  Invalidates
 * the forward pass.  Any other score refuses a layer with an edge bias by name when a pass is asked for; the bias is no parameter
 * (hnh_gat_optimizer_step does not touch it) unless hnh_gat_set_edge_bias_learned says so. */
int hnh_gat_set_edge_bias(hnh_gat* g, int layer, const hnh_vec* s, const hnh_vec* st);
/* A LEARNED edge bias (an addition; include/hnh_attn_edge_grad.h).  on != 0 makes the layer's bias a parameter: hnh_gat_backward also computes
 * dL/db_e = sum over the layer's heads of p_e (<dZ_i, V_j> - delta_i), heads added in the order 0 .. H-1, in S's order (from the backward row pass)
 * and in S^T's order (from the column pass), and hnh_gat_optimizer_step / hnh_gat_train_step update each copy of the bias from the gradient of its
 * own pass, with the other parameters' step count and hyper-parameters but NEVER with weight decay: an entry at -1e300 has gradient 0 and moments
 * 0 and stays -1e300 to the bit.  Every rank holds the bias of its own nonzeros: nothing is all-reduced.  Refused by name unless the layer has an
 * edge bias; clearing the bias clears the switch; switching off, clearing, or leaving score TRANSFORMER drops the gradient.  A layer whose bias is
 * not learned launches what it launched before.  hnh_gat_get_edge_bias copies the bias as it stands and hnh_gat_get_edge_bias_grad the gradient of
 * the last hnh_gat_backward into `out` (which = 0: S's order, a vector of hnh_vec_like's S layout; 1: S^T's); the gradient getter refuses before a
 * backward pass with the switch on and after anything that dropped the gradient.  A kernel library without the group: hnh_gat_backward and
 * hnh_gat_train_step name the missing symbol before anything is launched. */
int hnh_gat_set_edge_bias_learned(hnh_gat* g, int layer, int on);
int hnh_gat_get_edge_bias(hnh_gat* g, int layer, int which, hnh_vec* out);
int hnh_gat_get_edge_bias_grad(hnh_gat* g, int layer, int which, hnh_vec* out);
/* Output activation of a layer (an addition).  RELU (the default of hnh_gat_create on every layer): out = max(o, 0), everything above.  ELU:
 * out = o for o > 0 and expm1(o) otherwise.  IDENTITY: out = o.  The backward pass works from the stored output alone (include/hnh_grad.h,
 * hnh_act_grad_cols_f64).  A non-ReLU layer is supported with attention SOFTMAX, score DOT or ADDITIVE, any dropout rates, on 15d_fusion2
 * with c = 1; hnh_gat_forward / hnh_gat_backward / hnh_gat_train_step / hnh_gat_evaluate fail elsewhere before anything is launched, naming the
 * layer, the activation and the mode or the schedule, or hnh_act_grad_cols_f64 when the kernel library lacks it.  The published network is
 * ELU on the hidden layers and IDENTITY on the last one with HNH_GAT_HEADS_MEAN.  A change invalidates the stored forward pass; an unknown
 * mode or a layer out of range fails. */
#define HNH_GAT_ACT_RELU 0
#define HNH_GAT_ACT_ELU 1
#define HNH_GAT_ACT_IDENTITY 2
int hnh_gat_set_activation(hnh_gat* g, int layer, int mode);
/* Bias and skip connection of a layer (an addition; kernels: include/hnh_gat_skip.h, an optional group).  The layer's output becomes
 * out[:, block h] = act(o_h + r[:, block h] + b[block h]): r = 0 (NONE, the default), the layer input X (IDENTITY: input_features must equal
 * num_heads * features_per_head, refused here otherwise) or X W_res (PROJECTION: W_res is learned, input_features x (num_heads *
 * features_per_head), zero until set); b is the learned bias (num_heads * features_per_head entries; hnh_gat_set_bias with NULL switches
 * it off, the default).  All arrays are HOST memory, row-major.  Supported with attention SOFTMAX (every score, both backward modes, any
 * dropout the score allows, any activation) on 15d_fusion2 with c = 1; hnh_gat_forward / hnh_gat_backward / hnh_gat_train_step /
 * hnh_gat_evaluate fail elsewhere before anything is launched, naming the layer and the mode, the schedule, the shapes, or the missing symbol
 * when the kernel library lacks the group.  A layer with neither launches what it launched before.  Every setter invalidates the stored
 * forward pass.  After hnh_gat_backward the gradients (summed over all ranks like dW, the same on every rank) can be read;
 * hnh_gat_optimizer_step updates every enabled bias and W_res with the other parameters, weight decay included. */
#define HNH_GAT_RESIDUAL_NONE 0
#define HNH_GAT_RESIDUAL_IDENTITY 1
#define HNH_GAT_RESIDUAL_PROJECTION 2
int hnh_gat_set_residual(hnh_gat* g, int layer, int mode);
int hnh_gat_set_residual_weight(hnh_gat* g, int layer, const double* host);
int hnh_gat_get_residual_weight(hnh_gat* g, int layer, double* host);
int hnh_gat_get_residual_weight_grad(hnh_gat* g, int layer, double* host);
int hnh_gat_set_bias(hnh_gat* g, int layer, const double* host_or_null);
int hnh_gat_get_bias(hnh_gat* g, int layer, double* host);
int hnh_gat_get_bias_grad(hnh_gat* g, int layer, double* host);
/* Layer normalisation of a layer (an addition; kernels: include/hnh_gat_norm.h, an optional group).  With mode LAYER the layer's output becomes
 * out = act(gamma o xh + beta), xh = (z - mean(z)) / sqrt(var(z) + eps) over the WHOLE row z = o + r + b (all heads side by side, num_heads *
 * features_per_head values; the variance is the biased one): the post-norm block of the transformer, LayerNorm then the activation as in
 * TransformerConv / UniMP.  NONE is the default on every layer and launches what the layer launched before, bit for bit.  eps > 0 and finite
 * (1e-5 is customary); gamma = 1 and beta = 0 until hnh_gat_set_norm_weights, whose arrays (and the getters') are HOST memory of n = num_heads *
 * features_per_head doubles each; any other n fails.  Both are learned: after hnh_gat_backward, hnh_gat_get_norm_grad reads dL/dgamma and
 * dL/dbeta (summed over all ranks like dW, the same on every rank; it fails before a backward pass with the layer normalised), and
 * hnh_gat_optimizer_step / hnh_gat_train_step update them with the other parameters' step count and hyper-parameters but NEVER with weight
 * decay, which would pull gamma to 0.  A normalised layer keeps one more matrix of the layer output's size (the pre-normalisation rows) and two
 * doubles per row between the passes.  Supported where the activations are: attention SOFTMAX (every score, both backward modes, any dropout
 * the score allows, bias and both residuals) on 15d_fusion2 with c = 1, rows of at most HNH_NORM_MAX_COLS values; hnh_gat_forward /
 * hnh_gat_backward / hnh_gat_train_step / hnh_gat_evaluate fail elsewhere before anything is launched, naming the layer and the mode, the
 * schedule, the width, or the missing symbol when the kernel library lacks the group.  Every setter invalidates the stored forward pass; a
 * refused call leaves the object as it was. */
#define HNH_GAT_NORM_NONE 0
#define HNH_GAT_NORM_LAYER 1
int hnh_gat_set_norm(hnh_gat* g, int layer, int mode, double eps);
int hnh_gat_set_norm_weights(hnh_gat* g, int layer, const double* gamma_host, const double* beta_host, int64_t n);
int hnh_gat_get_norm_weights(hnh_gat* g, int layer, double* gamma_host, double* beta_host, int64_t n);
int hnh_gat_get_norm_grad(hnh_gat* g, int layer, double* dgamma_host, double* dbeta_host, int64_t n);
int hnh_gat_set_attn_vectors(hnh_gat* g, int layer, int head, const double* a1_host, const double* a2_host);
int hnh_gat_get_attn_grads(hnh_gat* g, int layer, int head, double* da1_host, double* da2_host);

/* Dropout (include/hnh_attn_dropout.h): rate attention_p on the normalised attention coefficients (score ADDITIVE only: requesting it
 * with score DOT makes hnh_gat_forward fail with an error naming score dot) and feature_p on every layer's input, both in [0, 1)
 * (anything else fails here), with masks recomputed in every pass from Philox-4x32-10 keyed by (seed, layer, head, global row, global
 * column): results do not depend on the rank count or on how a schedule splits a pass.  Rates (0, 0) are the default and launch the
 * kernels without dropout.  Both calls invalidate the stored forward pass, so hnh_gat_backward always differentiates the masks of the
 * forward pass it follows.  A kernel library without the group makes hnh_gat_forward fail with an error naming the missing symbol. */
int hnh_gat_set_dropout(hnh_gat* g, double attention_p, double feature_p, uint64_t seed);
int hnh_gat_set_dropout_seed(hnh_gat* g, uint64_t seed);
/* Word 0 of Philox-4x32-10 with counter (gi, gj, w2, stream) and key (seed & 0xffffffff, seed >> 32): the masks' generator, on the host
 * (stream 0: attention, w2 = layer * 65536 + head; stream 1: features, w2 = layer).  An entry is kept iff the word is >= floor(p 2^32). */
uint32_t hnh_dropout_word(uint64_t seed, uint32_t stream, uint32_t w2, uint32_t gi, uint32_t gj);

/* Training (an addition; kernels: include/hnh_train.h, an optional group — a kernel library without it makes hnh_gat_loss, hnh_gat_train_step,
 * hnh_gat_evaluate and hnh_gat_optimizer_step fail with an error naming the missing symbol).  Supported wherever hnh_gat_backward is.
 * Parameters can be read back: */
int hnh_gat_get_weight(hnh_gat* g, int layer, int head, double* host);                            /* row-major, hnh_gat_weight_shape */
int hnh_gat_get_attn_vectors(hnh_gat* g, int layer, int head, double* a1_host, double* a2_host); /* features_per_head doubles each */
/* Labels: n = M host entries in the operator's global row numbering (the rows of hnh_gat_get_output: block row + local row); a negative
 * label, or a row whose mask byte is 0 (mask_or_null == NULL: no mask), is not in the loss.  heads_mode MEAN: the classes are the last
 * layer's features_per_head and the logits the mean over its heads; CONCAT: num_heads * features_per_head classes, the row as it is.
 * (The published output layer averages raw head outputs: that is HNH_GAT_ACT_IDENTITY on the last layer.  With the default RELU there the
 * heads pass through the forward pass's ReLU before they are averaged.)  Each rank keeps its slice on the device; the labelled count is summed over the world once (collective).  A label
 * >= the class count, a mask without a labelled row or a wrong n fails and leaves the object as it was. */
#define HNH_GAT_HEADS_MEAN 0
#define HNH_GAT_HEADS_CONCAT 1
int hnh_gat_set_labels(hnh_gat* g, const int32_t* labels, const uint8_t* mask_or_null, int64_t n, int heads_mode);
/* Masked softmax cross-entropy of the stored forward pass (needs a valid one): *loss = the mean of -log p(label) and *accuracy = the share
 * of rows whose argmax is the label, over the labelled rows of the mask (NULL: the training rows of hnh_gat_set_labels), both summed over
 * the world.  grad_out_or_null receives dL/d(output) in the layout hnh_gat_backward takes. */
int hnh_gat_loss(hnh_gat* g, const uint8_t* mask_or_null, int64_t n, hnh_dense* grad_out_or_null, double* loss, double* accuracy);
/* kind ADAM: m = beta1 m + (1 - beta1) g', v = beta2 v + (1 - beta2) g'^2, p -= lr (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps);
 * SGD: v = momentum v + g', p -= lr v; g' = g + weight_decay p.  (Re)allocates zeroed moments and resets the step count t.
 * ADAMW (kernels: include/hnh_train_clip.h, an optional group — a kernel library without it makes hnh_gat_optimizer_step and
 * hnh_gat_train_step fail under this kind with an error naming the missing symbol): p = p (1 - lr weight_decay), then ADAM with g' = g
 * (torch.optim.AdamW).  The edge bias, gamma and beta are not decayed under any kind.
 * The step count restarts; the clip setting (hnh_gat_set_grad_clip) and the schedule (hnh_gat_set_lr_schedule) stay in place, and lr becomes
 * the schedule's base rate. */
#define HNH_GAT_OPTIMIZER_ADAM 0
#define HNH_GAT_OPTIMIZER_SGD 1
#define HNH_GAT_OPTIMIZER_ADAMW 2
int hnh_gat_set_optimizer(hnh_gat* g, int kind, double lr, double beta1, double beta2, double eps, double momentum, double weight_decay);
/* Applies the optimizer to the gradients of the last hnh_gat_backward — every W, a1, a2 with score ADDITIVE, and every enabled bias and
 * residual weight (weight decay applies to them as to every other tensor) — in one table-driven launch, and invalidates the stored forward pass.  The gradients are the same on every rank, so the parameters stay equal bit for bit. */
int hnh_gat_optimizer_step(hnh_gat* g);
/* One training step on the compute stream: [seed + 1 (mod 2^64) when a dropout rate is nonzero,] forward pass, loss over the training
 * rows into an internal gradient, backward pass, optimizer step.  *loss and *accuracy are those of the parameters BEFORE the update; reading
 * them is the call's only host synchronisation.  Fails before anything is launched when labels or optimizer are not set. */
int hnh_gat_train_step(hnh_gat* g, double* loss, double* accuracy);
/* Loss and accuracy over the mask's rows (NULL: the training rows) from a forward pass with both dropout rates 0 and no gradient.  Rates
 * and seed are restored; the stored forward pass stays invalid whenever a rate was nonzero. */
int hnh_gat_evaluate(hnh_gat* g, const uint8_t* mask_or_null, int64_t n, double* loss, double* accuracy);
/* The multi-label head (an addition; kernels: include/hnh_train_multilabel.h, an optional group — a kernel library without it makes
 * hnh_gat_loss, hnh_gat_train_step and hnh_gat_evaluate fail under this head with an error naming the missing symbol).  targets: n = M x
 * classes host bytes in {0, 1}, row-major, in the operator's global row numbering; classes must be what heads_mode gives (MEAN: the last
 * layer's features_per_head; CONCAT: num_heads * features_per_head).  mask_or_null: mask_n = M bytes, a row whose byte is 0 is not in the
 * loss (NULL: every row is).  pos_weight_or_null: `classes` doubles >= 0, the weight of a class's positive term (NULL: 1).  Afterwards
 * hnh_gat_loss / hnh_gat_train_step / hnh_gat_evaluate use the sigmoid head until the next hnh_gat_set_labels (the most recent of the two
 * calls decides): *loss = the mean over selected rows x classes of -w y log s(z) - (1 - y) log(1 - s(z)), z as under hnh_gat_set_labels,
 * and *accuracy = micro-averaged F1 = 2 tp / (2 tp + fp + fn) of the prediction z > 0 (0.0 when the denominator is 0), both over the whole
 * world; a mask given to hnh_gat_loss / hnh_gat_evaluate selects other rows of the same targets.  No limit on the row width applies.  Each
 * rank keeps its rows' bits on the device; the selected row count is summed over the world once (collective).  Any other target value
 * (named with its row and class), a wrong n or mask_n, a class count that does not match, a mask that selects no row or a weight that is
 * negative or not finite fails before anything is launched and leaves the object as it was. */
int hnh_gat_set_multilabel_targets(hnh_gat* g, const uint8_t* targets, int64_t n, int classes, const uint8_t* mask_or_null, int64_t mask_n,
                                   int heads_mode, const double* pos_weight_or_null);
/* (tp, fp, fn) of the last hnh_gat_loss / hnh_gat_evaluate / hnh_gat_train_step under the sigmoid head: counts of (row, class) pairs over
 * the whole world, exact.  Fails when the sigmoid head is not the one in use. */
int hnh_gat_multilabel_counts(hnh_gat* g, double* tp, double* fp, double* fn);
/* Gradient clipping by global norm (an addition; kernels: include/hnh_train_clip.h, an optional group — a kernel library without it makes
 * hnh_gat_optimizer_step and hnh_gat_train_step fail while clipping is on, before anything is launched, with an error naming the missing
 * symbol).  With max_norm > 0 every later step scales all gradients by min(1, max_norm / (norm + 1e-6)), norm = the 2-norm over every
 * learned tensor (torch.nn.utils.clip_grad_norm_): the replicated tensors counted once, a learned edge bias summed over the ranks that
 * hold its entries.  The norm and the coefficient stay on the device: hnh_gat_train_step keeps its single host synchronisation, and
 * parameters stay bit-equal across ranks.  A norm that is not finite gets no special handling.  max_norm == 0 (the default) switches
 * clipping off; a value that is negative, NaN or infinite fails and leaves the object as it was. */
int hnh_gat_set_grad_clip(hnh_gat* g, double max_norm);
/* *norm = the global gradient norm, before clipping, of the most recent step taken with clipping on; a device-to-host copy and a
 * synchronisation of its own.  Fails before the first such step. */
int hnh_gat_grad_norm(hnh_gat* g, double* norm);
/* A new base learning rate; unlike hnh_gat_set_optimizer it keeps the moments and the step count.  *lr of hnh_gat_learning_rate is the
 * rate the next step will use: base rate * factor(t), t = the 1-based number of that step.  Both need hnh_gat_set_optimizer first. */
int hnh_gat_set_learning_rate(hnh_gat* g, double lr);
int hnh_gat_learning_rate(hnh_gat* g, double* lr);
/* The schedule, host arithmetic in double on every step's rate: factor(t) = t / warmup_steps for t <= warmup_steps; afterwards CONSTANT
 * gives 1 (total_steps and min_factor are not used), LINEAR 1 - (1 - min_factor) (t - W) / (T - W) and COSINE min_factor + (1 - min_factor)
 * (1 + cos(pi (t - W) / (T - W))) / 2 with W = warmup_steps and T = total_steps, and min_factor for t > T.  LINEAR and COSINE need
 * T > W >= 0; min_factor must lie in [0, 1]; anything else fails and leaves the object as it was.  The default is CONSTANT without a
 * warm-up.  hnh_gat_set_optimizer restarts t and leaves the schedule in place. */
#define HNH_GAT_LR_CONSTANT 0
#define HNH_GAT_LR_LINEAR 1
#define HNH_GAT_LR_COSINE 2
int hnh_gat_set_lr_schedule(hnh_gat* g, int kind, int64_t warmup_steps, int64_t total_steps, double min_factor);

#ifdef __cplusplus
}
#endif
#endif /* HNH_DIST_H */
