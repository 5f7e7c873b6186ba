// Dense kernels of the GAT backward pass (include/hnh_grad.h).  The sparse side of that pass (SDDMM, SpMM) is the operator's own
// calls; what is here is the weight-gradient contraction X^T * dA and the small element-wise steps around it.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "hnh_ctx.hpp"
#include "hnh_grad.h"

namespace {

constexpr int kBlock = 256;

int ew_grid(int64_t n) {
    int64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---------------------------------------------------------------- C = A^T * B, split over K
// The tile machinery of gemm_f64_kernel (hnh_kernels.hip): block tile 128 x 128, K step 16, 4 waves in a 2 x 2 grid, each wave
// 4 x 4 accumulators of v_mfma_f64_16x16x4_f64, both tiles k-major in LDS ([k][m], [k][n]), the next K tile fetched into registers
// while the MFMAs of the current one run.  Fragment maps of the f64 MFMA:
//   A: lane l holds A[i = l & 15][k = l >> 4];  B: lane l holds B[k = l >> 4][j = l & 15];  C/D: register r of lane l is
//   C[row = (l >> 4) + 4 r][col = l & 15].
// What differs: A^T is stored K x M, so BOTH operands arrive k-major and both staging loads read 8 consecutive doubles of one row
// (16 threads per 128-wide row, 16 rows per K tile) and land in LDS with 16-byte stores, no transposition.
// K is long and M x N small (the weight gradient: 1024 x 1024 from K = 2^18 is 64 tiles for 256 CUs), so the K range is cut into
// `slices` consecutive pieces of kc rows: workgroup (tile, slice) writes its partial tile into slab `slice` of the workspace, and
// gemm_tn_reduce_kernel adds the slabs in slice order (or the single slice writes C directly).
// Placement: the workgroups of ONE slice go to one XCD (blockIdx.x % 8) — its tiles read the same K rows of A and B, which that
// XCD's L2 then serves to all of them — and slices are spread over the XCDs.  A speed choice only: results do not depend on it.
typedef double d4_t __attribute__((ext_vector_type(4)));
constexpr int kTile = 128, kBK = 16, kLd = kTile + 4, kXcds = 8;
constexpr int kTnThreads = 256;
constexpr int kTargetGroups = 512;  // two 4-wave workgroups per CU on 256 CUs
constexpr int kMinKTilesPerSlice = 32;
constexpr int kMaxSlices = 64;

struct TnPlan {
    int64_t row_blocks = 0, col_blocks = 0, tiles = 0, slices = 1, kc = 0;
};

// The split depends on the shape only (never on the device or the environment): results are bit-identical run to run and box to box.
TnPlan tn_plan(int64_t M, int64_t N, int64_t K) {
    TnPlan p;
    p.row_blocks = (M + kTile - 1) / kTile;
    p.col_blocks = (N + kTile - 1) / kTile;
    p.tiles = p.row_blocks * p.col_blocks;
    const int64_t kt = (K + kBK - 1) / kBK;
    int64_t s = 1;
    if (p.tiles > 0 && p.tiles < kTargetGroups) {
        s = (kTargetGroups + p.tiles - 1) / p.tiles;
        const int64_t by_k = kt / kMinKTilesPerSlice;
        if (s > by_k) s = by_k;
        if (s > kMaxSlices) s = kMaxSlices;
        if (s < 1) s = 1;
    }
    const int64_t per = kt > 0 ? (kt + s - 1) / s : 1;  // K tiles per slice
    p.slices = kt > 0 ? (kt + per - 1) / per : 1;        // no empty slice
    p.kc = per * kBK;
    return p;
}

__global__ __launch_bounds__(kTnThreads) void gemm_tn_f64_kernel(int64_t M, int64_t N, int64_t K, const double* __restrict__ A,
                                                                 int64_t lda, const double* __restrict__ B, int64_t ldb,
                                                                 double* __restrict__ out, int64_t ld_out, int64_t slab_stride,
                                                                 int64_t kc, int64_t tiles, int64_t col_blocks, int64_t groups,
                                                                 int64_t per_xcd, bool vec_ok) {
    __shared__ double As[2][kBK][kLd];
    __shared__ double Bs[2][kBK][kLd];
    const int64_t id = blockIdx.x;
    const int64_t v = (id % kXcds) * per_xcd + id / kXcds;
    if (v >= groups) return;
    const int64_t slice = v / tiles, tile = v % tiles;
    const int64_t row0 = (tile / col_blocks) * kTile, col0 = (tile % col_blocks) * kTile;
    const int64_t kbeg = slice * kc;
    const int64_t kend = (kbeg + kc < K) ? kbeg + kc : K;
    double* __restrict__ dst = out + slice * slab_stride;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    d4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (d4_t){0.0, 0.0, 0.0, 0.0};

    // global -> register staging: K row sk of both operands, 8 consecutive columns from sc
    const int sk = tid >> 4, sc = (tid & 15) * 8;
    const bool interior = vec_ok && row0 + kTile <= M && col0 + kTile <= N;
    double ra[8], rb[8];
    auto fetch = [&](int64_t k0) {
        const int64_t gk = k0 + sk;
        if (interior && k0 + kBK <= kend) {
            const double* ap = A + gk * lda + row0 + sc;
            const double* bp = B + gk * ldb + col0 + sc;
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const double2 va = *reinterpret_cast<const double2*>(ap + q);
                const double2 vb = *reinterpret_cast<const double2*>(bp + q);
                ra[q] = va.x; ra[q + 1] = va.y;
                rb[q] = vb.x; rb[q + 1] = vb.y;
            }
        } else {
            const bool kin = gk < kend;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int64_t gm = row0 + sc + q, gn = col0 + sc + q;
                ra[q] = (kin && gm < M) ? A[gk * lda + gm] : 0.0;
                rb[q] = (kin && gn < N) ? B[gk * ldb + gn] : 0.0;
            }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 8; q += 2) {
            *reinterpret_cast<double2*>(&As[buf][sk][sc + q]) = make_double2(ra[q], ra[q + 1]);
            *reinterpret_cast<double2*>(&Bs[buf][sk][sc + q]) = make_double2(rb[q], rb[q + 1]);
        }
    };

    const int64_t ktiles = (kend > kbeg) ? (kend - kbeg + kBK - 1) / kBK : 0;
    if (ktiles > 0) {
        fetch(kbeg);
        stage(0);
    }
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;
    for (int64_t t = 0; t < ktiles; t++) {
        const int buf = (int)(t & 1);
        if (t + 1 < ktiles) fetch(kbeg + (t + 1) * kBK);  // in flight during the MFMAs below
#pragma unroll
        for (int kk = 0; kk < kBK; kk += 4) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = As[buf][kk + fk][wm + i * 16 + fr];
#pragma unroll
            for (int j = 0; j < 4; j++) b[j] = Bs[buf][kk + fk][wn + j * 16 + fr];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < ktiles) stage(buf ^ 1);  // the other buffer: its readers finished before the previous barrier
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t row = row0 + wm + i * 16 + fk + 4 * r, col = col0 + wn + j * 16 + fr;
                if (row < M && col < N) dst[row * ld_out + col] = acc[i][j][r];
            }
}

// C[i, j] = sum over s = 0 .. slices-1, in that order, of slab s (M x N, leading dimension N)
__global__ __launch_bounds__(kBlock) void gemm_tn_reduce_kernel(double* __restrict__ C, int64_t ldc, const double* __restrict__ work,
                                                                int64_t M, int64_t N, int64_t slices) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = M * N;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        double s = work[i];
        for (int64_t q = 1; q < slices; q++) s += work[q * total + i];
        C[(i / N) * ldc + i % N] = s;
    }
}

// ---------------------------------------------------------------- element-wise steps of the backward pass
__global__ __launch_bounds__(kBlock) void leaky_relu_grad_kernel(double* __restrict__ e, double* __restrict__ d, double alpha, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double x = e[i];
        e[i] = fmax(x, 0.0) + fmin(x, 0.0) * alpha;  // the forward's activation, bit for bit (hnh_leaky_relu_f64)
        d[i] = x > 0.0 ? d[i] : d[i] * alpha;
    }
}

__global__ __launch_bounds__(kBlock) void relu_grad_cols_kernel(double* __restrict__ dz, int64_t ld_dz, const double* __restrict__ g,
                                                                int64_t ld_g, const double* __restrict__ out, int64_t ld_out, int64_t col0,
                                                                int64_t rows, int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / cols, c = i % cols;
        dz[r * ld_dz + c] = out[r * ld_out + col0 + c] > 0.0 ? g[r * ld_g + col0 + c] : 0.0;
    }
}

// dZ and delta of one head from G and the STORED output in one pass (hnh_act_grad_cols_f64).  A group of 2^lpr_log2 lanes owns a row and
// walks its columns W doubles per lane (W = 2: 16-byte lanes): 256 >> lpr_log2 short rows per workgroup, one wave per wide row.  delta is
// the lanes' partial sums (each in column order) added by an xor butterfly inside the group, a fixed order: no atomics, no LDS.
//   relu:     dz = out > 0 ? g : 0,                 term = dz * out
//   identity: dz = g,                               term = g * out
//   elu:      out >= 0: dz = g, term = g * out;     out < 0: u = 1 + out, dz = g * u, term = dz * log1p(out), 0 where u == 0 (a unit
//             saturated at -1 has dz = 0, and 0 * -inf must not become a NaN)
template <int W>
__global__ __launch_bounds__(kBlock) void act_grad_cols_kernel(double* __restrict__ dz, int64_t ld_dz, double* __restrict__ delta,
                                                               const double* __restrict__ g, int64_t ld_g, const double* __restrict__ out,
                                                               int64_t ld_out, int64_t col0, int64_t rows, int cols, int act, int lpr_log2) {
    const int lpr = 1 << lpr_log2;
    const int tid = threadIdx.x, lig = tid & (lpr - 1);
    const int64_t row = (int64_t)blockIdx.x * (kBlock >> lpr_log2) + (tid >> lpr_log2);
    if (row >= rows) return;  // (whole groups leave: the butterfly below stays inside a group)
    const double* __restrict__ gr = g + row * ld_g + col0;
    const double* __restrict__ orow = out + row * ld_out + col0;
    double* __restrict__ zr = dz + row * ld_dz;
    double s = 0.0;
    for (int c = lig * W; c < cols; c += lpr * W) {
        double gv[W], ov[W], zv[W];
        if constexpr (W == 2) {
            const double2 a = *reinterpret_cast<const double2*>(gr + c);
            const double2 b = *reinterpret_cast<const double2*>(orow + c);
            gv[0] = a.x; gv[1] = a.y;
            ov[0] = b.x; ov[1] = b.y;
        } else {
            gv[0] = gr[c];
            ov[0] = orow[c];
        }
#pragma unroll
        for (int w = 0; w < W; w++) {
            const double o = ov[w];
            if (act == HNH_ACT_RELU) {
                zv[w] = o > 0.0 ? gv[w] : 0.0;
                s = fma(zv[w], o, s);
            } else if (act == HNH_ACT_IDENTITY || o >= 0.0) {
                zv[w] = gv[w];
                s = fma(gv[w], o, s);
            } else {
                const double u = 1.0 + o;
                zv[w] = gv[w] * u;
                if (u > 0.0) s = fma(zv[w], log1p(o), s);
            }
        }
        if constexpr (W == 2) *reinterpret_cast<double2*>(zr + c) = make_double2(zv[0], zv[1]);
        else zr[c] = zv[0];
    }
    for (int m = lpr >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lig == 0) delta[row] = s;
}

__global__ __launch_bounds__(kBlock) void sum3_cols_kernel(double* __restrict__ dst, int64_t ld, int64_t col0, const double* __restrict__ x,
                                                           const double* __restrict__ y, const double* __restrict__ z, int64_t rows,
                                                           int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / cols, c = i % cols;
        dst[r * ld + col0 + c] = (x[i] + y[i]) + z[i];
    }
}

__global__ __launch_bounds__(kBlock) void transpose_into_kernel(double* __restrict__ dst, int64_t ld, int64_t row0, const double* __restrict__ w,
                                                                int64_t rows, int64_t cols) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t c = i / rows, r = i % rows;  // consecutive threads write consecutive columns of one row of dst
        dst[(row0 + c) * ld + r] = w[r * cols + c];
    }
}

}  // namespace

extern "C" {

int64_t hnh_gemm_tn_f64_workspace(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const TnPlan p = tn_plan(M, N, K);
    return p.slices > 1 ? p.slices * M * N : 0;
}

int hnh_gemm_tn_f64(hnh_ctx* ctx, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb,
                    double* C, int64_t ldc, double* work, int64_t work_doubles, int stream) {
    HNH_ENTER(ctx, stream);
    if (M < 0 || N < 0 || K < 0) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gemm_tn_f64: negative size");
    if (lda < M || ldb < N || ldc < N) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gemm_tn_f64: leading dimension smaller than the width");
    if (M == 0 || N == 0) return HNH_OK;
    if (!C) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gemm_tn_f64: null pointer");
    if (K == 0) {  // an empty sum
        HNH_TRY_HIP(ctx, hipMemset2DAsync(C, sizeof(double) * (size_t)ldc, 0, sizeof(double) * (size_t)N, (size_t)M, ctx->streams[stream]));
        return HNH_OK;
    }
    if (!A || !B) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gemm_tn_f64: null pointer");
    const TnPlan p = tn_plan(M, N, K);
    const int64_t need = p.slices > 1 ? p.slices * M * N : 0;
    if (need > 0 && (!work || work_doubles < need))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gemm_tn_f64: workspace smaller than hnh_gemm_tn_f64_workspace()");
    const int64_t groups = p.tiles * p.slices;
    const int64_t per_xcd = (groups + kXcds - 1) / kXcds;
    const int64_t grid = per_xcd * kXcds;
    if (grid > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "hnh_gemm_tn_f64: matrix too large");
    const bool vec_ok = (lda % 2 == 0) && (ldb % 2 == 0) && aligned16(A) && aligned16(B);
    hnh::WideLaunch wide(ctx, stream);  // a dense contraction wants every matrix core
    if (wide.status != HNH_OK) return wide.status;
    double* out = p.slices > 1 ? work : C;
    const int64_t ld_out = p.slices > 1 ? N : ldc, slab = p.slices > 1 ? M * N : 0;
    hipLaunchKernelGGL(gemm_tn_f64_kernel, dim3((unsigned)grid), dim3(kTnThreads), 0, wide.stream(), M, N, K, A, lda, B, ldb, out, ld_out,
                       slab, p.kc, p.tiles, p.col_blocks, groups, per_xcd, vec_ok);
    int rc = hnh::check_hip(ctx, hipGetLastError(), "gemm_tn_f64_kernel launch");
    if (rc == HNH_OK && p.slices > 1) {
        hipLaunchKernelGGL(gemm_tn_reduce_kernel, dim3(ew_grid(M * N)), dim3(kBlock), 0, wide.stream(), C, ldc, work, M, N, p.slices);
        rc = hnh::check_hip(ctx, hipGetLastError(), "gemm_tn_reduce_kernel launch");
    }
    return wide.finish(rc);
}

int hnh_leaky_relu_grad_f64(hnh_ctx* ctx, double* e_to_a, double* da_to_de, double alpha, int64_t n, int stream) {
    HNH_ENTER(ctx, stream);
    if (n < 0) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_leaky_relu_grad_f64: negative size");
    if (n == 0) return HNH_OK;
    if (!e_to_a || !da_to_de) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_leaky_relu_grad_f64: null pointer");
    hipLaunchKernelGGL(leaky_relu_grad_kernel, dim3(ew_grid(n)), dim3(kBlock), 0, ctx->streams[stream], e_to_a, da_to_de, alpha, n);
    return hnh::check_hip(ctx, hipGetLastError(), "leaky_relu_grad_kernel launch");
}

int hnh_relu_grad_cols_f64(hnh_ctx* ctx, double* dZ, int64_t ld_dz, const double* G, int64_t ld_g, const double* out, int64_t ld_out,
                           int64_t col0, int64_t rows, int64_t cols, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || col0 < 0 || ld_dz < cols || col0 + cols > ld_g || col0 + cols > ld_out)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_relu_grad_cols_f64: bad shape");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dZ || !G || !out) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_relu_grad_cols_f64: null pointer");
    hipLaunchKernelGGL(relu_grad_cols_kernel, dim3(ew_grid(rows * cols)), dim3(kBlock), 0, ctx->streams[stream], dZ, ld_dz, G, ld_g, out,
                       ld_out, col0, rows, cols);
    return hnh::check_hip(ctx, hipGetLastError(), "relu_grad_cols_kernel launch");
}

int hnh_act_grad_cols_f64(hnh_ctx* ctx, double* dZ, int64_t ld_dz, double* delta, const double* G, int64_t ld_g, const double* out,
                          int64_t ld_out, int64_t col0, int64_t rows, int64_t cols, int act, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || col0 < 0 || ld_dz < cols || col0 + cols > ld_g || col0 + cols > ld_out || cols > 0x7fffffffLL)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_act_grad_cols_f64: bad shape");
    if (act != HNH_ACT_RELU && act != HNH_ACT_ELU && act != HNH_ACT_IDENTITY)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_act_grad_cols_f64: unknown activation " + std::to_string(act) + " (relu = 0, elu = 1, identity = 2)");
    if (rows == 0) return HNH_OK;
    if (!delta || (cols > 0 && (!dZ || !G || !out))) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_act_grad_cols_f64: null pointer");
    // 16-byte lanes where every row's column block starts on a 16-byte boundary in all three matrices
    const bool vec = cols % 2 == 0 && col0 % 2 == 0 && ld_dz % 2 == 0 && ld_g % 2 == 0 && ld_out % 2 == 0 && aligned16(dZ) && aligned16(G) && aligned16(out);
    const int w = vec ? 2 : 1;
    int lpr_log2 = 0;  // the smallest power-of-two group that covers the row in one trip, at most one wave
    while (lpr_log2 < 6 && ((int64_t)w << lpr_log2) < cols) lpr_log2++;
    const int64_t groups = kBlock >> lpr_log2, blocks = (rows + groups - 1) / groups;
    if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "hnh_act_grad_cols_f64: too many rows for one launch");
    if (vec)
        hipLaunchKernelGGL(act_grad_cols_kernel<2>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->streams[stream], dZ, ld_dz, delta, G, ld_g, out, ld_out,
                           col0, rows, (int)cols, act, lpr_log2);
    else
        hipLaunchKernelGGL(act_grad_cols_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->streams[stream], dZ, ld_dz, delta, G, ld_g, out, ld_out,
                           col0, rows, (int)cols, act, lpr_log2);
    return hnh::check_hip(ctx, hipGetLastError(), "act_grad_cols_kernel launch");
}

int hnh_sum3_cols_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, int64_t col0, const double* x, const double* y, const double* z,
                      int64_t rows, int64_t cols, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || col0 < 0 || col0 + cols > ld_dst) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_sum3_cols_f64: bad shape");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dst || !x || !y || !z) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_sum3_cols_f64: null pointer");
    hipLaunchKernelGGL(sum3_cols_kernel, dim3(ew_grid(rows * cols)), dim3(kBlock), 0, ctx->streams[stream], dst, ld_dst, col0, x, y, z, rows,
                       cols);
    return hnh::check_hip(ctx, hipGetLastError(), "sum3_cols_kernel launch");
}

int hnh_transpose_into_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, int64_t row0, const double* W, int64_t rows, int64_t cols,
                           int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || row0 < 0 || ld_dst < rows) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_transpose_into_f64: bad shape");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dst || !W) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_transpose_into_f64: null pointer");
    hipLaunchKernelGGL(transpose_into_kernel, dim3(ew_grid(rows * cols)), dim3(kBlock), 0, ctx->streams[stream], dst, ld_dst, row0, W, rows,
                       cols);
    return hnh::check_hip(ctx, hipGetLastError(), "transpose_into_kernel launch");
}

}  // extern "C"

#include "hnh_train_kernels.hpp"  // the training step (include/hnh_train.h): cross-entropy head and optimizer
#include "hnh_train_clip_kernels.hpp"  // gradient clipping and AdamW (include/hnh_train_clip.h): the sum of squares and the clipped optimizer step
#include "hnh_gat_skip_kernels.hpp"  // bias and skip connections (include/hnh_gat_skip.h): the dense kernels
#include "hnh_gat_norm_kernels.hpp"  // layer normalisation (include/hnh_gat_norm.h): the two dense row passes
#include "hnh_multilabel_kernels.hpp"  // the multi-label head (include/hnh_train_multilabel.h): sigmoid cross-entropy and the micro-F1 counts
#include "hnh_als_implicit_kernels.hpp"  // implicit-feedback ALS (include/hnh_als_implicit.h): the Gram term and the guarded CG update of a row tile
#include "hnh_topk_kernels.hpp"  // top-k recommendation (include/hnh_topk.h): fused scores and selection, the merge of lists, a row gather
#include "hnh_rank_kernels.hpp"  // exact item ranks (include/hnh_rank.h): counting on the score tile, the scores of pairs, the subtraction of excluded entries
