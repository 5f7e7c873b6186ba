// Bias and skip connections of the GAT layers (include/hnh_gat_skip.h): the dense kernels.  Included at the end of hnh_grad.hip, whose
// helpers (kBlock, ew_grid, aligned16) they use; the finishing launches' side of the group, HNH_ATTN_ADDEND, lives with the attention
// passes in hnh_kernels.hip.  All three are one pass over their operands at 16 bytes per lane where the layout allows:
//   addend  writes rows x cols, reads rows x cols of res when there is one (bias stays in cache)
//   grad    hnh_act_grad_cols_f64's traffic (G and out read, dZ written) plus a second dZ store and a read of res when there is one
//   colsum  reads rows x cols once; the partial sums are (row ranges) x cols, at most kColsumRanges rows of them
#pragma once
#include "hnh_gat_skip.h"

namespace {

template <int W>
__global__ __launch_bounds__(kBlock) void skip_addend_cols_kernel(double* __restrict__ dst, int64_t ld_dst, int64_t col0, const double* __restrict__ res,
                                                                  int64_t ld_res, const double* __restrict__ bias, int64_t rows, int64_t cols) {
    const int64_t per_row = cols / W;  // (W == 2: cols is even)
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / per_row, c = (i % per_row) * W;
        double v[W];
#pragma unroll
        for (int w = 0; w < W; w++) v[w] = 0.0;
        if (res != nullptr) {
            if constexpr (W == 2) {
                const double2 t = *reinterpret_cast<const double2*>(res + r * ld_res + c);
                v[0] = t.x; v[1] = t.y;
            } else {
                v[0] = res[r * ld_res + c];
            }
        }
        if (bias != nullptr) {
#pragma unroll
            for (int w = 0; w < W; w++) v[w] += bias[c + w];
        }
        double* d = dst + r * ld_dst + col0 + c;
        if constexpr (W == 2) *reinterpret_cast<double2*>(d) = make_double2(v[0], v[1]);
        else *d = v[0];
    }
}

// act_grad_cols_kernel (hnh_grad.hip) with the addend taken out of the recovered pre-activation: the same lane layout, the same dZ,
// the same summation order.  res / bias / dz_all may be null (a wave-uniform choice).
template <int W>
__global__ __launch_bounds__(kBlock) void skip_grad_cols_kernel(double* __restrict__ dz, int64_t ld_dz, double* __restrict__ dz_all, int64_t ld_all,
                                                                double* __restrict__ delta, const double* __restrict__ g, int64_t ld_g,
                                                                const double* __restrict__ out, int64_t ld_out, int64_t col0,
                                                                const double* __restrict__ res, int64_t ld_res, const double* __restrict__ bias,
                                                                int64_t rows, int cols, int act, int lpr_log2) {
    const int lpr = 1 << lpr_log2;
    const int tid = threadIdx.x, lig = tid & (lpr - 1);
    const int64_t row = (int64_t)blockIdx.x * (kBlock >> lpr_log2) + (tid >> lpr_log2);
    if (row >= rows) return;  // (whole groups leave: the butterfly below stays inside a group)
    const double* __restrict__ gr = g + row * ld_g + col0;
    const double* __restrict__ orow = out + row * ld_out + col0;
    const double* __restrict__ rr = res != nullptr ? res + row * ld_res : nullptr;
    double* __restrict__ zr = dz + row * ld_dz;
    double* __restrict__ za = dz_all != nullptr ? dz_all + row * ld_all + col0 : nullptr;
    double s = 0.0;
    for (int c = lig * W; c < cols; c += lpr * W) {
        double gv[W], ov[W], zv[W], rv[W], bv[W];
#pragma unroll
        for (int w = 0; w < W; w++) { rv[w] = 0.0; bv[w] = 0.0; }
        if constexpr (W == 2) {
            const double2 a = *reinterpret_cast<const double2*>(gr + c);
            const double2 b = *reinterpret_cast<const double2*>(orow + c);
            gv[0] = a.x; gv[1] = a.y;
            ov[0] = b.x; ov[1] = b.y;
            if (rr != nullptr) {
                const double2 t = *reinterpret_cast<const double2*>(rr + c);
                rv[0] = t.x; rv[1] = t.y;
            }
            if (bias != nullptr) {
                const double2 t = *reinterpret_cast<const double2*>(bias + c);
                bv[0] = t.x; bv[1] = t.y;
            }
        } else {
            gv[0] = gr[c];
            ov[0] = orow[c];
            if (rr != nullptr) rv[0] = rr[c];
            if (bias != nullptr) bv[0] = bias[c];
        }
#pragma unroll
        for (int w = 0; w < W; w++) {
            const double o = ov[w];
            if (act == HNH_ACT_RELU) {
                zv[w] = o > 0.0 ? gv[w] : 0.0;
                if (o > 0.0) s = fma(zv[w], (o - rv[w]) - bv[w], s);  // (elsewhere dZ = 0: no term, whatever the addend holds)
            } else if (act == HNH_ACT_IDENTITY || o >= 0.0) {
                zv[w] = gv[w];
                s = fma(gv[w], (o - rv[w]) - bv[w], s);
            } else {
                const double u = 1.0 + o;
                zv[w] = gv[w] * u;
                if (u > 0.0) s = fma(zv[w], (log1p(o) - rv[w]) - bv[w], s);
            }
        }
        if constexpr (W == 2) {
            *reinterpret_cast<double2*>(zr + c) = make_double2(zv[0], zv[1]);
            if (za != nullptr) *reinterpret_cast<double2*>(za + c) = make_double2(zv[0], zv[1]);
        } else {
            zr[c] = zv[0];
            if (za != nullptr) za[c] = zv[0];
        }
    }
    for (int m = lpr >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lig == 0) delta[row] = s;
}

// Column sums in two launches.  The rows are cut into `ranges` consecutive ranges of `per` rows (a function of the row count alone);
// workgroup (column tile, range) is 32 lanes x 8 row phases: phase p adds rows first + p, first + p + 8, .. of its range in that order,
// W columns per lane, then lane (0, x) adds the eight phase sums in phase order and stores the range's partial row.  The second launch
// adds the ranges front to back.  Neither the tile width nor W changes the order in which a column's rows are added.
constexpr int kColsumRanges = 512, kColsumMinRows = 256, kColsumLanes = 32, kColsumPhases = kBlock / kColsumLanes;

struct ColsumPlan {
    int64_t ranges = 1, per = 0;
};
ColsumPlan colsum_plan(int64_t rows) {
    ColsumPlan p;
    int64_t n = (rows + kColsumMinRows - 1) / kColsumMinRows;
    if (n > kColsumRanges) n = kColsumRanges;
    if (n < 1) n = 1;
    p.per = rows > 0 ? (rows + n - 1) / n : 0;
    p.ranges = rows > 0 ? (rows + p.per - 1) / p.per : 1;  // no empty range
    return p;
}

template <int W>
__global__ __launch_bounds__(kBlock) void colsum_ranges_kernel(double* __restrict__ work, const double* __restrict__ src, int64_t ld, int64_t rows,
                                                               int64_t cols, int64_t per) {
    __shared__ double part[kColsumPhases][kColsumLanes * W];
    const int x = threadIdx.x % kColsumLanes, p = threadIdx.x / kColsumLanes;
    const int64_t c = ((int64_t)blockIdx.x * kColsumLanes + x) * W;
    const int64_t first = (int64_t)blockIdx.y * per;
    const int64_t last = first + per < rows ? first + per : rows;
    const bool live = c < cols;  // (W == 2: cols is even)
    double s[W];
#pragma unroll
    for (int w = 0; w < W; w++) s[w] = 0.0;
    if (live) {
        for (int64_t r = first + p; r < last; r += kColsumPhases) {
            if constexpr (W == 2) {
                const double2 t = *reinterpret_cast<const double2*>(src + r * ld + c);
                s[0] += t.x;
                s[1] += t.y;
            } else {
                s[0] += src[r * ld + c];
            }
        }
    }
#pragma unroll
    for (int w = 0; w < W; w++) part[p][x * W + w] = s[w];
    __syncthreads();
    if (p == 0 && live) {
#pragma unroll
        for (int w = 0; w < W; w++) {
            double t = part[0][x * W + w];
#pragma unroll
            for (int q = 1; q < kColsumPhases; q++) t += part[q][x * W + w];
            work[(int64_t)blockIdx.y * cols + c + w] = t;
        }
    }
}

__global__ __launch_bounds__(kBlock) void colsum_finish_kernel(double* __restrict__ out, const double* __restrict__ work, int64_t cols, int64_t ranges) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= cols) return;
    double s = work[c];
    for (int64_t q = 1; q < ranges; q++) s += work[q * cols + c];
    out[c] = s;
}

}  // namespace

extern "C" {

int hnh_skip_addend_cols_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, int64_t col0, const double* res, int64_t ld_res, const double* bias,
                             int64_t rows, int64_t cols, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || col0 < 0 || col0 + cols > ld_dst || (res != nullptr && ld_res < cols))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_skip_addend_cols_f64: bad shape");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dst) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_skip_addend_cols_f64: null pointer");
    if (res != nullptr && (const double*)dst == res) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_skip_addend_cols_f64: res aliases the destination");
    const bool vec = cols % 2 == 0 && col0 % 2 == 0 && ld_dst % 2 == 0 && aligned16(dst) && (res == nullptr || (ld_res % 2 == 0 && aligned16(res)));
    hipStream_t st = ctx->streams[stream];
    if (vec)
        hipLaunchKernelGGL(skip_addend_cols_kernel<2>, dim3(ew_grid(rows * (cols / 2))), dim3(kBlock), 0, st, dst, ld_dst, col0, res, ld_res, bias, rows, cols);
    else
        hipLaunchKernelGGL(skip_addend_cols_kernel<1>, dim3(ew_grid(rows * cols)), dim3(kBlock), 0, st, dst, ld_dst, col0, res, ld_res, bias, rows, cols);
    return hnh::check_hip(ctx, hipGetLastError(), "skip_addend_cols_kernel launch");
}

int hnh_skip_grad_cols_f64(hnh_ctx* ctx, double* dZ, int64_t ld_dz, double* dZ_all, int64_t ld_all, double* delta, const double* G, int64_t ld_g,
                           const double* out, int64_t ld_out, int64_t col0, const double* res, int64_t ld_res, const double* bias, int64_t rows,
                           int64_t cols, int act, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || col0 < 0 || ld_dz < cols || col0 + cols > ld_g || col0 + cols > ld_out || cols > 0x7fffffffLL ||
        (dZ_all != nullptr && col0 + cols > ld_all) || (res != nullptr && ld_res < cols))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_skip_grad_cols_f64: bad shape");
    if (act != HNH_ACT_RELU && act != HNH_ACT_ELU && act != HNH_ACT_IDENTITY)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_skip_grad_cols_f64: unknown activation " + std::to_string(act) + " (relu = 0, elu = 1, identity = 2)");
    if (rows == 0) return HNH_OK;
    if (!delta || (cols > 0 && (!dZ || !G || !out))) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_skip_grad_cols_f64: null pointer");
    if (dZ_all != nullptr && (dZ_all == dZ || (const double*)dZ_all == G || (const double*)dZ_all == out))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_skip_grad_cols_f64: dZ_all aliases an operand");
    // 16-byte lanes where every row's column block starts on a 16-byte boundary in every matrix in use
    const bool vec = cols % 2 == 0 && col0 % 2 == 0 && ld_dz % 2 == 0 && ld_g % 2 == 0 && ld_out % 2 == 0 && aligned16(dZ) && aligned16(G) && aligned16(out) &&
                     (dZ_all == nullptr || (ld_all % 2 == 0 && aligned16(dZ_all))) && (res == nullptr || (ld_res % 2 == 0 && aligned16(res))) &&
                     (bias == nullptr || aligned16(bias));
    const int w = vec ? 2 : 1;
    int lpr_log2 = 0;  // the smallest power-of-two group that covers the row in one trip, at most one wave
    while (lpr_log2 < 6 && ((int64_t)w << lpr_log2) < cols) lpr_log2++;
    const int64_t groups = kBlock >> lpr_log2, blocks = (rows + groups - 1) / groups;
    if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "hnh_skip_grad_cols_f64: too many rows for one launch");
    hipStream_t st = ctx->streams[stream];
    if (vec)
        hipLaunchKernelGGL(skip_grad_cols_kernel<2>, dim3((unsigned)blocks), dim3(kBlock), 0, st, dZ, ld_dz, dZ_all, ld_all, delta, G, ld_g, out, ld_out, col0,
                           res, ld_res, bias, rows, (int)cols, act, lpr_log2);
    else
        hipLaunchKernelGGL(skip_grad_cols_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, dZ, ld_dz, dZ_all, ld_all, delta, G, ld_g, out, ld_out, col0,
                           res, ld_res, bias, rows, (int)cols, act, lpr_log2);
    return hnh::check_hip(ctx, hipGetLastError(), "skip_grad_cols_kernel launch");
}

int64_t hnh_colsum_f64_workspace(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0) return 0;
    return colsum_plan(rows).ranges * cols;
}

int hnh_colsum_f64(hnh_ctx* ctx, double* out, const double* src, int64_t ld, int64_t rows, int64_t cols, double* work, int64_t work_doubles,
                   int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || ld < cols) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_colsum_f64: bad shape");
    if (cols == 0) return HNH_OK;
    if (!out) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_colsum_f64: null pointer");
    hipStream_t st = ctx->streams[stream];
    if (rows == 0) {  // an empty sum
        HNH_TRY_HIP(ctx, hipMemsetAsync(out, 0, sizeof(double) * (size_t)cols, st));
        return HNH_OK;
    }
    const ColsumPlan p = colsum_plan(rows);
    if (!src || !work || work_doubles < p.ranges * cols)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_colsum_f64: null pointer or a workspace smaller than hnh_colsum_f64_workspace()");
    if ((const double*)out == src || out == work) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_colsum_f64: out aliases an operand");
    const bool vec = cols % 2 == 0 && ld % 2 == 0 && aligned16(src);
    const int64_t tile = kColsumLanes * (vec ? 2 : 1), tiles = (cols + tile - 1) / tile;
    if (tiles > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "hnh_colsum_f64: too many columns for one launch");
    const dim3 grid((unsigned)tiles, (unsigned)p.ranges);
    if (vec) hipLaunchKernelGGL(colsum_ranges_kernel<2>, grid, dim3(kBlock), 0, st, work, src, ld, rows, cols, p.per);
    else hipLaunchKernelGGL(colsum_ranges_kernel<1>, grid, dim3(kBlock), 0, st, work, src, ld, rows, cols, p.per);
    if (int rc = hnh::check_hip(ctx, hipGetLastError(), "colsum_ranges_kernel launch")) return rc;
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)((cols + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, out, work, cols, p.ranges);
    return hnh::check_hip(ctx, hipGetLastError(), "colsum_finish_kernel launch");
}

}  // extern "C"
