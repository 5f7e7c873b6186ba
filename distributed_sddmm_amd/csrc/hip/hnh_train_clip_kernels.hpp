// Gradient clipping by global norm and AdamW (include/hnh_train_clip.h).  Included at the end of hnh_grad.hip, behind hnh_train_kernels.hpp.
//
// grad_sumsq_kernel: a streaming read.  A tensor is cut into UNITS, two neighbouring doubles of a row where its width is even and one
// double otherwise (a tensor whose pitch is its width counts as one long row), and gets a run of workgroups of its own: ceil(units /
// (kBlock * kSumsqUnitsPerThread)) of them, at most kSumsqMaxBlocks.  Thread j of the run takes units j, j + S, j + 2 S, .. (S = the
// run's threads) into ONE accumulator with explicit fmas; the row and column of a unit are stepped with the host's (S / width, S %
// width), so no thread divides more than once.  A unit of two is one 16-byte load where base and pitch are even, two 8-byte loads
// otherwise: the same elements into the same additions, so the result does not depend on where a tensor lies.  The workgroup's sum: xor
// butterflies inside a wave (every lane ends with the wave's sum), then the four waves in order into work[workgroup].
// grad_sumsq_finish_kernel: thread t adds partials t, t + 256, ..; a tree adds the threads; out = [base +] [prev +] that.
// optim_step_clip_kernel: optim_step_kernel with coef * g for g; the coefficient is uniform over the launch, so one branch picks a loop
// that takes g itself (coef == 1: the parent's operations, and its bits) or one that takes the rounded product.
#pragma once
#include <vector>
#include "hnh_train_clip.h"

namespace {

constexpr int kSumsqUnitsPerThread = 8;
constexpr int kSumsqMaxBlocks = 2048;  // of one tensor: 2048 * 256 threads with 16-byte loads in flight cover the device's latency

struct SumsqEntry {
    const double* g;
    int64_t ld, width, units;  // pitch in doubles; units in a row; units in all
    int64_t step_r, step_c;    // (run's threads) / width and % width
    int first_block, blocks;   // the tensor's run of workgroups
    int unit, vec;             // doubles in a unit (1 | 2); whether a unit is one 16-byte load
};

struct SumsqTable {
    SumsqEntry t[HNH_OPTIM_MAX_TENSORS];
    int n;
};

typedef double sumsq_d2_t __attribute__((ext_vector_type(2)));

template <int UNIT, bool VEC>
__device__ inline double sumsq_thread(const SumsqEntry& t, int64_t first) {
    double acc = 0.0;
    if (first >= t.units) return acc;
    int64_t r = first / t.width, c = first % t.width;
#pragma unroll 4
    for (int64_t i = first; i < t.units; i += (int64_t)t.blocks * kBlock) {
        const double* q = t.g + r * t.ld + c * UNIT;
        if (UNIT == 2) {
            double x, y;
            if (VEC) {
                const sumsq_d2_t v = *reinterpret_cast<const sumsq_d2_t*>(q);
                x = v.x;
                y = v.y;
            } else {
                x = q[0];
                y = q[1];
            }
            acc = __builtin_fma(x, x, acc);
            acc = __builtin_fma(y, y, acc);
        } else {
            const double x = q[0];
            acc = __builtin_fma(x, x, acc);
        }
        r += t.step_r;
        c += t.step_c;
        if (c >= t.width) {
            c -= t.width;
            r += 1;
        }
    }
    return acc;
}

__global__ __launch_bounds__(kBlock) void grad_sumsq_kernel(SumsqTable tab, double* __restrict__ work) {
    __shared__ double waves[kBlock / 64];
    int k = 0;
    while (k + 1 < tab.n && (int)blockIdx.x >= tab.t[k + 1].first_block) k++;  // (uniform: the tensor of this workgroup)
    const SumsqEntry t = tab.t[k];
    const int64_t first = (int64_t)((int)blockIdx.x - t.first_block) * kBlock + threadIdx.x;
    double acc;
    if (t.unit == 2) acc = t.vec ? sumsq_thread<2, true>(t, first) : sumsq_thread<2, false>(t, first);
    else acc = sumsq_thread<1, false>(t, first);
    for (int off = 32; off > 0; off >>= 1) acc += xor_shuffle(acc, off);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kBlock / 64; w++) s += waves[w];
        work[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kBlock) void grad_sumsq_finish_kernel(double* out, const double* prev, const double* base, const double* __restrict__ work,
                                                                   int blocks) {
    __shared__ double s[kBlock];
    double a = 0.0;
    for (int k = threadIdx.x; k < blocks; k += kBlock) a += work[k];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int half = kBlock / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double v = s[0];
        if (prev != nullptr) v = *prev + v;
        if (base != nullptr) v = *base + v;
        *out = v;
    }
}

// One element's update with every rounding written out (contraction is off in here, and each fused step is an explicit fma): the
// operations optim_step_kernel compiles to, which the compiler otherwise chooses anew in every context it meets the expression in.
//     gd = fma(wd, p, g)                                  AdamW: p = p (1 - lr wd), gd = g
//     m = fma(b1, m, (1 - b1) gd);  v = fma(b2, v, gd ((1 - b2) gd));  p = p - (lr (m / bias1)) / (sqrt(v / bias2) + eps)
//     SGD: v = fma(momentum, v, gd);  p = fma(-lr, v, p)
template <int KIND, bool SCALED>
__device__ inline void optim_clip_loop(const hnh_optim_tensor& t, const hnh_optim& hy, double coef) {
#pragma clang fp contract(off)
    const int64_t total = t.rows * t.cols, stride = (int64_t)gridDim.x * kBlock;
    const double one_b1 = 1.0 - hy.beta1, one_b2 = 1.0 - hy.beta2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / t.cols, c = i % t.cols;
        double* pp = t.p + r * t.ld_p + c;
        double p = *pp;
        const double g = SCALED ? coef * t.g[r * t.ld_g + c] : t.g[r * t.ld_g + c];
        double gd;
        if (KIND == HNH_OPTIM_ADAMW) {
            p = p * (1.0 - hy.lr * hy.weight_decay);
            gd = g;
        } else {
            gd = __builtin_fma(hy.weight_decay, p, g);
        }
        if (KIND != HNH_OPTIM_SGD) {
            const double m = __builtin_fma(hy.beta1, t.m[i], one_b1 * gd);
            const double v = __builtin_fma(hy.beta2, t.v[i], gd * (one_b2 * gd));
            t.m[i] = m;
            t.v[i] = v;
            *pp = p - (hy.lr * (m / hy.bias1)) / (sqrt(v / hy.bias2) + hy.eps);
        } else {
            const double v = __builtin_fma(hy.momentum, t.v[i], gd);
            t.v[i] = v;
            *pp = __builtin_fma(-hy.lr, v, p);
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void optim_step_clip_kernel(OptimTable tab, hnh_optim hy, const double* __restrict__ sumsq, int nsums, double max_norm) {
    const hnh_optim_tensor t = tab.t[blockIdx.y];
    double coef = 1.0;
    if (sumsq != nullptr) {
        double total = 0.0;
        for (int q = 0; q < nsums; q++) total += sumsq[q];
        const double c = max_norm / (sqrt(total) + 1e-6);
        coef = c > 1.0 ? 1.0 : c;  // (a NaN stays a NaN)
    }
    if (coef == 1.0) optim_clip_loop<KIND, false>(t, hy, coef);
    else optim_clip_loop<KIND, true>(t, hy, coef);
}

// The launches of one part of a table (at most HNH_OPTIM_MAX_TENSORS entries): the kernel's table and its workgroup count, functions of
// rows, cols and ld_g alone but for the load width.  Returns 0, 1 (a bad shape or pitch) or 2 (with `pointers`: a null g).
int sumsq_plan(const hnh_optim_tensor* tensors, int count, bool pointers, SumsqTable* tab, int* blocks) {
    tab->n = 0;
    *blocks = 0;
    for (int k = 0; k < count; k++) {
        const hnh_optim_tensor& t = tensors[k];
        if (t.rows < 0 || t.cols < 0 || t.ld_g < t.cols) return 1;
        const int64_t total = t.rows * t.cols;
        if (total == 0) continue;
        if (pointers && !t.g) return 2;
        SumsqEntry e = {};
        const bool dense = t.ld_g == t.cols || t.rows == 1;  // one long row
        const int64_t width = dense ? total : t.cols;
        e.g = t.g;
        e.ld = dense ? total : t.ld_g;
        e.unit = width % 2 == 0 ? 2 : 1;
        e.width = width / e.unit;
        e.units = total / e.unit;
        e.vec = e.unit == 2 && aligned16(t.g) && e.ld % 2 == 0;
        int64_t b = (e.units + (int64_t)kBlock * kSumsqUnitsPerThread - 1) / ((int64_t)kBlock * kSumsqUnitsPerThread);
        if (b > kSumsqMaxBlocks) b = kSumsqMaxBlocks;
        e.blocks = (int)b;
        e.first_block = *blocks;
        e.step_r = (b * kBlock) / e.width;
        e.step_c = (b * kBlock) % e.width;
        *blocks += e.blocks;
        tab->t[tab->n++] = e;
    }
    return 0;
}

int sumsq_parts(int n) { return (n + HNH_OPTIM_MAX_TENSORS - 1) / HNH_OPTIM_MAX_TENSORS; }

}  // namespace

extern "C" {

// work: [0, parts) the running sum behind every part, then the partials of the part in flight (stream order frees them for the next one)
int64_t hnh_grad_sumsq_f64_workspace(const hnh_optim_tensor* tensors, int n) {
    if (n < 0 || (n > 0 && !tensors)) return -1;
    int64_t most = 0;
    for (int first = 0; first < n; first += HNH_OPTIM_MAX_TENSORS) {
        SumsqTable tab;
        int blocks = 0;
        if (sumsq_plan(tensors + first, n - first < HNH_OPTIM_MAX_TENSORS ? n - first : HNH_OPTIM_MAX_TENSORS, false, &tab, &blocks) != 0) return -1;
        most = blocks > most ? blocks : most;
    }
    const int64_t need = sumsq_parts(n) + most;
    return need < 1 ? 1 : need;
}

int hnh_grad_sumsq_f64(hnh_ctx* ctx, const hnh_optim_tensor* tensors, int n, int accumulate, double* result, double* work, int64_t work_doubles,
                       int stream) {
    HNH_ENTER(ctx, stream);
    if (n < 0 || (n > 0 && !tensors)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_grad_sumsq_f64: null table or negative count");
    const int64_t need = hnh_grad_sumsq_f64_workspace(tensors, n);
    if (need < 0) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_grad_sumsq_f64: bad shape or pitch");
    if (!result || !work || work_doubles < need) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_grad_sumsq_f64: null result or short workspace");
    std::vector<SumsqTable> tabs;  // the parts that hold elements
    std::vector<int> blocks;
    for (int first = 0; first < n; first += HNH_OPTIM_MAX_TENSORS) {
        SumsqTable tab;
        int b = 0;
        if (sumsq_plan(tensors + first, n - first < HNH_OPTIM_MAX_TENSORS ? n - first : HNH_OPTIM_MAX_TENSORS, true, &tab, &b) != 0)
            return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_grad_sumsq_f64: null pointer");
        if (b == 0) continue;
        tabs.push_back(tab);
        blocks.push_back(b);
    }
    const size_t parts = tabs.size();
    const double* partials = work + sumsq_parts(n);
    const double* none = nullptr;
    const double* base = accumulate ? result : none;
    hipStream_t st = ctx->streams[stream];
    if (parts == 0) {  // result = [result +] 0
        hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(kBlock), 0, st, result, none, base, partials, 0);
        return hnh::check_hip(ctx, hipGetLastError(), "grad_sumsq_finish_kernel launch");
    }
    for (size_t j = 0; j < parts; j++) {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks[j]), dim3(kBlock), 0, st, tabs[j], work + sumsq_parts(n));
        if (int rc = hnh::check_hip(ctx, hipGetLastError(), "grad_sumsq_kernel launch")) return rc;
        const bool last = j + 1 == parts;
        const double* prev = j > 0 ? work + (j - 1) : none;
        hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(kBlock), 0, st, last ? result : work + j, prev, last ? base : none, partials, blocks[j]);
        if (int rc = hnh::check_hip(ctx, hipGetLastError(), "grad_sumsq_finish_kernel launch")) return rc;
    }
    return HNH_OK;
}

int hnh_optim_step_clip_f64(hnh_ctx* ctx, const hnh_optim_tensor* tensors, int n, const hnh_optim* hyper, const double* sumsq, int nsums,
                            double max_norm, int stream) {
    HNH_ENTER(ctx, stream);
    if (n < 0 || (n > 0 && !tensors) || !hyper) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_clip_f64: null table or negative count");
    const int kind = hyper->kind;
    if (kind != HNH_OPTIM_ADAM && kind != HNH_OPTIM_SGD && kind != HNH_OPTIM_ADAMW)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_clip_f64: unknown optimizer kind " + std::to_string(kind));
    if (kind != HNH_OPTIM_SGD && !(hyper->bias1 > 0.0 && hyper->bias2 > 0.0))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_clip_f64: Adam's bias corrections must be positive");
    if (sumsq != nullptr && (nsums < 1 || nsums > HNH_CLIP_MAX_SUMS || !(max_norm >= 0.0)))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_clip_f64: nsums outside 1 .. HNH_CLIP_MAX_SUMS, or max_norm negative or NaN");
    for (int k = 0; k < n; k++) {
        const hnh_optim_tensor& t = tensors[k];
        if (t.rows < 0 || t.cols < 0 || t.ld_p < t.cols || t.ld_g < t.cols) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_clip_f64: bad shape or pitch");
        if (t.rows * t.cols > 0 && (!t.p || !t.g || !t.v || (kind != HNH_OPTIM_SGD && !t.m)))
            return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_optim_step_clip_f64: null pointer");
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
        hipStream_t st = ctx->streams[stream];
        if (kind == HNH_OPTIM_ADAM) hipLaunchKernelGGL(optim_step_clip_kernel<HNH_OPTIM_ADAM>, grid, dim3(kBlock), 0, st, tab, *hyper, sumsq, nsums, max_norm);
        else if (kind == HNH_OPTIM_SGD) hipLaunchKernelGGL(optim_step_clip_kernel<HNH_OPTIM_SGD>, grid, dim3(kBlock), 0, st, tab, *hyper, sumsq, nsums, max_norm);
        else hipLaunchKernelGGL(optim_step_clip_kernel<HNH_OPTIM_ADAMW>, grid, dim3(kBlock), 0, st, tab, *hyper, sumsq, nsums, max_norm);
        if (int rc = hnh::check_hip(ctx, hipGetLastError(), "optim_step_clip_kernel launch")) return rc;
    }
    return HNH_OK;
}

}  // extern "C"
