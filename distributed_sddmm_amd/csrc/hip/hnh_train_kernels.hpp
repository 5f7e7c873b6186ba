// The GAT's training step (include/hnh_train.h).  Included at the end of hnh_grad.hip.
//
// xent_rows_kernel: a GROUP of g lanes owns a row (g = the power of two that covers heads * classes, 4 .. 64: a wave takes one wide row
// or several short ones).  The group stages its row in LDS with one coalesced read, builds z (the mean over heads) beside it, takes max /
// argmax from LDS, turns z into exp(z - max) in place while it sums (one exp per class) and writes G = scale (e / sum - [c == label]) with one
// coalesced store: one trip to memory each way.  A group lies inside one wave and its LDS region is its own, so the steps are ordered by
// wave-level synchronisation, not by block barriers.  Cross-lane steps are xor butterflies inside the group (a fixed order; every lane
// ends with the result).  A workgroup's rows add up in group order into ONE partial pair; xent_finish_kernel adds the partials in a fixed
// order.  optim_step_kernel: blockIdx.y picks the tensor of the table in the kernel arguments, blockIdx.x strides over its elements.
#pragma once
#include "hnh_train.h"

namespace {

constexpr int kXentMaxBlocks = 4096;  // partial pairs in the workspace
constexpr int kXentLdsBytes = 65536;  // dynamic LDS a workgroup may ask for without an attribute

template <typename T>
__device__ inline T xor_shuffle(T v, int off) {
    return __shfl_xor(v, off, 64);
}

// Orders the LDS traffic of one wave: a group lies inside a wave and its LDS region is its own, so no round needs the other waves.
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kBlock) void xent_rows_kernel(const double* out, int64_t ld_out, const int* __restrict__ labels, int64_t rows, int heads,
                                                           int classes, double inv_n, double* G, int64_t ld_g, double* __restrict__ work, int g,
                                                           int region) {
    extern __shared__ double xent_lds[];
    const int n = heads * classes;
    const int groups = (int)blockDim.x / g;  // rows of a workgroup per round
    const int grp = (int)threadIdx.x / g, l = (int)threadIdx.x % g;
    double* row = xent_lds + (size_t)grp * region;  // n doubles
    double* z = heads > 1 ? row + n : row;           // classes doubles (the row itself with one head)
    double* part = xent_lds + (size_t)groups * region;  // per group: loss, correct, bad labels
    const double inv_heads = 1.0 / (double)heads;
    const int cstep = g % classes;
    double loss = 0.0, correct = 0.0, bad = 0.0;  // (lane 0 of the group keeps them)
    for (int64_t base = (int64_t)blockIdx.x * groups; base < rows; base += (int64_t)gridDim.x * groups) {
        const int64_t r = base + grp;
        int label = r < rows ? labels[r] : -1;
        if (label >= classes) {
            if (l == 0) bad += 1.0;
            label = -1;
        }
        const bool live = label >= 0;  // (uniform over the group)
        if (live)
            for (int j = l; j < n; j += g) row[j] = out[r * ld_out + j];
        wave_sync();
        if (live && heads > 1)
            for (int c = l; c < classes; c += g) {
                double s = 0.0;
                for (int h = 0; h < heads; h++) s += row[h * classes + c];
                z[c] = s * inv_heads;
            }
        wave_sync();
        double mx = -INFINITY;
        int arg = 0x7fffffff;
        if (live)
            for (int c = l; c < classes; c += g) {
                const double v = z[c];
                if (v > mx || arg == 0x7fffffff) {  // (ascending c: a tie keeps the lowest index)
                    mx = v;
                    arg = c;
                }
            }
        for (int off = g >> 1; off > 0; off >>= 1) {
            const double ov = xor_shuffle(mx, off);
            const int oa = xor_shuffle(arg, off);
            if (oa != 0x7fffffff && (arg == 0x7fffffff || ov > mx || (ov == mx && oa < arg))) {
                mx = ov;
                arg = oa;
            }
        }
        const double zl = live ? z[label] : 0.0;  // (read by every lane before any lane overwrites z)
        wave_sync();
        double sum = 0.0;
        if (live)
            for (int c = l; c < classes; c += g) {  // z becomes exp(z - max): one exp per class
                const double e = exp(z[c] - mx);
                z[c] = e;
                sum += e;
            }
        for (int off = g >> 1; off > 0; off >>= 1) sum += xor_shuffle(sum, off);
        if (live && l == 0) {
            loss -= (zl - mx) - log(sum);
            correct += arg == label ? 1.0 : 0.0;
        }
        wave_sync();
        if (G != nullptr && r < rows) {
            if (live) {
                const double scale = inv_n * inv_heads, inv_sum = 1.0 / sum;
                int c = l % classes;  // the class of column j, stepped along with j
                for (int j = l; j < n; j += g) {
                    G[r * ld_g + j] = scale * (z[c] * inv_sum - (c == label ? 1.0 : 0.0));
                    c += cstep;
                    if (c >= classes) c -= classes;
                }
            } else {
                for (int j = l; j < n; j += g) G[r * ld_g + j] = 0.0;
            }
        }
        wave_sync();  // (the next round stages into the same region)
    }
    if (l == 0) {
        part[grp * 3] = loss;
        part[grp * 3 + 1] = correct;
        part[grp * 3 + 2] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int k = 0; k < groups; k++) {
            a += part[k * 3];
            b += part[k * 3 + 1];
            c += part[k * 3 + 2];
        }
        work[blockIdx.x] = a;
        work[gridDim.x + blockIdx.x] = b;
        work[2 * gridDim.x + blockIdx.x] = c;
    }
}

// result = the partial pairs of `blocks` workgroups in a fixed order: thread t adds partials t, t + 256, .. and a tree adds the threads
__global__ __launch_bounds__(kBlock) void xent_finish_kernel(double* __restrict__ result, const double* __restrict__ work, int blocks) {
    __shared__ double s[3][kBlock];
    for (int q = 0; q < 3; q++) {
        double a = 0.0;
        for (int k = threadIdx.x; k < blocks; k += kBlock) a += work[q * blocks + k];
        s[q][threadIdx.x] = a;
    }
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int q = 0; q < 3; q++) s[q][threadIdx.x] += s[q][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool bad = s[2][0] > 0.0;
        result[0] = bad ? NAN : s[0][0];
        result[1] = bad ? -s[2][0] : s[1][0];
    }
}

struct OptimTable {
    hnh_optim_tensor t[HNH_OPTIM_MAX_TENSORS];
};

template <int KIND>
__global__ __launch_bounds__(kBlock) void optim_step_kernel(OptimTable tab, hnh_optim hy) {
    const hnh_optim_tensor t = tab.t[blockIdx.y];
    const int64_t total = t.rows * t.cols, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / t.cols, c = i % t.cols;
        double* pp = t.p + r * t.ld_p + c;
        const double p = *pp;
        const double gd = t.g[r * t.ld_g + c] + hy.weight_decay * p;
        if (KIND == HNH_OPTIM_ADAM) {
            const double m = hy.beta1 * t.m[i] + (1.0 - hy.beta1) * gd;
            const double v = hy.beta2 * t.v[i] + (1.0 - hy.beta2) * gd * gd;
            t.m[i] = m;
            t.v[i] = v;
            *pp = p - hy.lr * (m / hy.bias1) / (sqrt(v / hy.bias2) + hy.eps);
        } else {
            const double v = hy.momentum * t.v[i] + gd;
            t.v[i] = v;
            *pp = p - hy.lr * v;
        }
    }
}

int xent_blocks(int64_t rows) { return (int)(rows < 1 ? 1 : (rows > kXentMaxBlocks ? kXentMaxBlocks : rows)); }

}  // namespace

extern "C" {

int64_t hnh_xent_rows_f64_workspace(int64_t rows) { return 3 * (int64_t)xent_blocks(rows); }

int hnh_xent_rows_f64(hnh_ctx* ctx, const double* out, int64_t ld_out, const int32_t* labels, int64_t rows, int heads, int classes,
                      double inv_n, double* G, int64_t ld_g, double* result, double* work, int64_t work_doubles, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || heads < 1 || classes < 1) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_xent_rows_f64: bad shape");
    if ((int64_t)heads * classes > HNH_XENT_MAX_WIDTH)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_xent_rows_f64: rows of heads * classes = " + std::to_string((int64_t)heads * classes) +
                                                   " doubles exceed HNH_XENT_MAX_WIDTH = " + std::to_string(HNH_XENT_MAX_WIDTH));
    const int n = heads * classes;
    if (ld_out < n || (G && ld_g < n)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_xent_rows_f64: bad pitch");
    if (!result || !work || work_doubles < hnh_xent_rows_f64_workspace(rows)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_xent_rows_f64: null result or short workspace");
    if (rows > 0 && (!out || !labels)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_xent_rows_f64: null pointer");
    int g = 4;
    while (g < 64 && g < n) g *= 2;
    const int region = n + (heads > 1 ? classes : 0);
    // the widest workgroup (a multiple of a wave) whose groups' regions and partials fit the LDS
    int threads = kBlock;
    while (threads > 64 && (size_t)(threads / g) * (region + 3) * sizeof(double) > (size_t)kXentLdsBytes) threads /= 2;
    const int groups = threads / g;
    const size_t lds = (size_t)groups * (region + 3) * sizeof(double);
    if (lds > (size_t)kXentLdsBytes) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_xent_rows_f64: a row does not fit the LDS");
    int64_t want = (rows + groups - 1) / groups;
    const int blocks = xent_blocks(want);
    hipLaunchKernelGGL(xent_rows_kernel, dim3(blocks), dim3(threads), lds, ctx->streams[stream], out, ld_out, labels, rows, heads, classes, inv_n, G, ld_g,
                       work, g, region);
    if (int rc = hnh::check_hip(ctx, hipGetLastError(), "xent_rows_kernel launch")) return rc;
    hipLaunchKernelGGL(xent_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->streams[stream], result, work, blocks);
    return hnh::check_hip(ctx, hipGetLastError(), "xent_finish_kernel launch");
}

int hnh_optim_step_f64(hnh_ctx* ctx, const hnh_optim_tensor* tensors, int n, const hnh_optim* hyper, int stream) {
    HNH_ENTER(ctx, stream);
    if (n < 0 || (n > 0 && !tensors) || !hyper) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_f64: null table or negative count");
    if (hyper->kind != HNH_OPTIM_ADAM && hyper->kind != HNH_OPTIM_SGD)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_f64: unknown optimizer kind " + std::to_string(hyper->kind));
    if (hyper->kind == HNH_OPTIM_ADAM && !(hyper->bias1 > 0.0 && hyper->bias2 > 0.0))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_f64: Adam's bias corrections must be positive");
    for (int k = 0; k < n; k++) {
        const hnh_optim_tensor& t = tensors[k];
        if (t.rows < 0 || t.cols < 0 || t.ld_p < t.cols || t.ld_g < t.cols) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_f64: bad shape or pitch");
        if (t.rows * t.cols > 0 && (!t.p || !t.g || !t.v || (hyper->kind == HNH_OPTIM_ADAM && !t.m)))
            return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_f64: null pointer");
    }
    for (int first = 0; first < n; first += HNH_OPTIM_MAX_TENSORS) {
        const int count = n - first < HNH_OPTIM_MAX_TENSORS ? n - first : HNH_OPTIM_MAX_TENSORS;
        OptimTable tab = {};
        int64_t most = 0;
        for (int k = 0; k < count; k++) {
            tab.t[k] = tensors[first + k];
            const int64_t e = tab.t[k].rows * tab.t[k].cols;
            most = e > most ? e : most;
        }
        if (most == 0) continue;
        int64_t bx = (most + kBlock - 1) / kBlock;
        if (bx > 1024) bx = 1024;
        const dim3 grid((unsigned)bx, (unsigned)count);
        if (hyper->kind == HNH_OPTIM_ADAM) hipLaunchKernelGGL(optim_step_kernel<HNH_OPTIM_ADAM>, grid, dim3(kBlock), 0, ctx->streams[stream], tab, *hyper);
        else hipLaunchKernelGGL(optim_step_kernel<HNH_OPTIM_SGD>, grid, dim3(kBlock), 0, ctx->streams[stream], tab, *hyper);
        if (int rc = hnh::check_hip(ctx, hipGetLastError(), "optim_step_kernel launch")) return rc;
    }
    return HNH_OK;
}

}  // extern "C"
