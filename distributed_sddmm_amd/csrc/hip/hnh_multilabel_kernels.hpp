// The GAT's multi-label head (include/hnh_train_multilabel.h).  Included at the end of hnh_grad.hip.
//
// bce_rows_kernel: a GROUP of g lanes owns a row (g = the power of two that covers `classes`, 4 .. 64: a wave takes one wide row, looping
// over its classes in steps of 64, or several short ones).  A lane owns classes l, l + g, ..: it reads its class's `heads` values (the lanes
// of a group read consecutive doubles of one head block: coalesced 8-byte accesses), forms z, the loss term and the three counts in
// registers and writes G to the elements it has read, so nothing is staged, no lane needs another lane's value and G may alias out.  The
// target word of 32 classes is one broadcast read.  The pass is bound by the latency of a row's dependent loads, not by arithmetic: a lane
// takes two classes a step with all their loads ahead of the first store, and the next row's mask byte is read a row ahead.  Every lane keeps its four sums over all its rows; a workgroup adds them with one tree
// in LDS into ONE set of partials, and bce_finish_kernel adds the partials in a fixed order.
#pragma once
#include "hnh_train_multilabel.h"

namespace {

constexpr int kBceMaxBlocks = 2048;  // sets of partials in the workspace (256 CUs x 8 workgroups)

// One class of one row: adds its loss term and its counts and returns dL/dz.  sig = s(|z|) and 1 - s(|z|) come from e = exp(-|z|) without a
// cancellation; s (1 - y + w y) - w y is s for y = 0 and -w (1 - s) for y = 1.  A NaN z stays a NaN through sp.
__device__ __forceinline__ double bce_term(double z, bool y, double w, double scale, double& loss, double& tp, double& fp, double& fn) {
    const double e = exp(-fabs(z)), sp = log1p(e);
    const double t = 1.0 / (1.0 + e), p = e * t;
    loss += y ? w * (fmax(-z, 0.0) + sp) : fmax(z, 0.0) + sp;
    const bool pred = z > 0.0;
    tp += (y && pred) ? 1.0 : 0.0;
    fp += (!y && pred) ? 1.0 : 0.0;
    fn += (y && !pred) ? 1.0 : 0.0;
    return y ? -(scale * w) * (z >= 0.0 ? p : t) : scale * (z >= 0.0 ? t : p);
}

__global__ __launch_bounds__(kBlock) void bce_rows_kernel(const double* out, int64_t ld_out, const uint32_t* __restrict__ targets, int64_t ld_t,
                                                          const uint8_t* __restrict__ row_mask, const double* __restrict__ pos_weight, int64_t rows,
                                                          int heads, int classes, double inv_n, double* G, int64_t ld_g, double* __restrict__ work,
                                                          int g) {
    __shared__ double s[4][kBlock];
    const int groups = kBlock / g;  // rows of a workgroup per round
    const int grp = (int)threadIdx.x / g, l = (int)threadIdx.x % g;
    const double inv_heads = 1.0 / (double)heads, scale = inv_n * inv_heads;
    const int64_t stride = (int64_t)gridDim.x * groups;
    double loss = 0.0, tp = 0.0, fp = 0.0, fn = 0.0;
    int64_t r = (int64_t)blockIdx.x * groups + grp;
    uint8_t live = r < rows ? row_mask[r] : 0;  // (uniform over the group)
    while (r < rows) {
        const int64_t next = r + stride;
        const uint8_t next_live = next < rows ? row_mask[next] : 0;  // (in flight while this row is worked on)
        const double* orow = out + r * ld_out;
        double* grow = G != nullptr ? G + r * ld_g : nullptr;
        if (live == 0) {
            if (grow != nullptr)
                for (int c = l; c < classes; c += g)
                    for (int h = 0; h < heads; h++) grow[(int64_t)h * classes + c] = 0.0;
        } else {
            const uint32_t* trow = targets + r * ld_t;
            // two classes a step, c0 and c1 = c0 + g: every load of both before the first store (G may alias out, but a lane writes only the
            // elements it has read, so its loads of c1 may pass its stores of c0)
            for (int c0 = l; c0 < classes; c0 += 2 * g) {
                const int c1 = c0 + g;
                const bool two = c1 < classes;
                const int c1s = two ? c1 : c0;
                double sum0 = 0.0, sum1 = 0.0;
                for (int h = 0; h < heads; h++) {
                    sum0 += orow[(int64_t)h * classes + c0];
                    sum1 += orow[(int64_t)h * classes + c1s];
                }
                const bool y0 = ((trow[c0 >> 5] >> (c0 & 31)) & 1u) != 0, y1 = ((trow[c1s >> 5] >> (c1s & 31)) & 1u) != 0;
                const double w0 = pos_weight != nullptr ? pos_weight[c0] : 1.0, w1 = pos_weight != nullptr ? pos_weight[c1s] : 1.0;
                const double g0 = bce_term(sum0 * inv_heads, y0, w0, scale, loss, tp, fp, fn);
                double g1 = 0.0;
                if (two) g1 = bce_term(sum1 * inv_heads, y1, w1, scale, loss, tp, fp, fn);
                if (grow != nullptr) {
                    for (int h = 0; h < heads; h++) grow[(int64_t)h * classes + c0] = g0;
                    if (two)
                        for (int h = 0; h < heads; h++) grow[(int64_t)h * classes + c1] = g1;
                }
            }
        }
        r = next;
        live = next_live;
    }
    s[0][threadIdx.x] = loss;
    s[1][threadIdx.x] = tp;
    s[2][threadIdx.x] = fp;
    s[3][threadIdx.x] = fn;
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int q = 0; q < 4; q++) s[q][threadIdx.x] += s[q][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < 4) work[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s[threadIdx.x][0];
}

// result = the four partials of `blocks` workgroups in a fixed order: thread t adds partials t, t + 256, .. and a tree adds the threads
__global__ __launch_bounds__(kBlock) void bce_finish_kernel(double* __restrict__ result, const double* __restrict__ work, int blocks) {
    __shared__ double s[4][kBlock];
    for (int q = 0; q < 4; q++) {
        double a = 0.0;
        for (int k = threadIdx.x; k < blocks; k += kBlock) a += work[q * blocks + k];
        s[q][threadIdx.x] = a;
    }
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int q = 0; q < 4; q++) s[q][threadIdx.x] += s[q][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < 4) result[threadIdx.x] = s[threadIdx.x][0];
}

int bce_blocks(int64_t want) { return (int)(want < 1 ? 1 : (want > kBceMaxBlocks ? kBceMaxBlocks : want)); }

}  // namespace

extern "C" {

int64_t hnh_bce_rows_f64_workspace(int64_t rows) { return 4 * (int64_t)bce_blocks(rows); }

int hnh_bce_rows_f64(hnh_ctx* ctx, const double* out, int64_t ld_out, const uint32_t* targets, int64_t ld_t, const uint8_t* row_mask,
                     const double* pos_weight, int64_t rows, int heads, int classes, double inv_n, double* G, int64_t ld_g, double* result,
                     double* work, int64_t work_doubles, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || heads < 1 || classes < 1) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_bce_rows_f64: bad shape");
    const int64_t n = (int64_t)heads * classes;
    if (ld_out < n || (G && ld_g < n) || ld_t < ((int64_t)classes + 31) / 32) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_bce_rows_f64: bad pitch");
    if (!result || !work || work_doubles < hnh_bce_rows_f64_workspace(rows)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_bce_rows_f64: null result or short workspace");
    if (rows > 0 && (!out || !targets || !row_mask)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_bce_rows_f64: null pointer");
    int g = 4;
    while (g < 64 && g < classes) g *= 2;
    const int groups = kBlock / g;
    const int blocks = bce_blocks((rows + groups - 1) / groups);  // (never more than bce_blocks(rows): the workspace holds them)
    hipLaunchKernelGGL(bce_rows_kernel, dim3(blocks), dim3(kBlock), 0, ctx->streams[stream], out, ld_out, targets, ld_t, row_mask, pos_weight, rows, heads,
                       classes, inv_n, G, ld_g, work, g);
    if (int rc = hnh::check_hip(ctx, hipGetLastError(), "bce_rows_kernel launch")) return rc;
    hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->streams[stream], result, work, blocks);
    return hnh::check_hip(ctx, hipGetLastError(), "bce_finish_kernel launch");
}

}  // extern "C"
