// Layer normalisation of the GAT layers (include/hnh_gat_norm.h): two dense row passes.  Included at the end of hnh_grad.hip, whose
// helpers (kBlock, aligned16) they use.  A row stays in registers between its reductions and its store:
//   forward   reads z once and writes out (16 B per element), plus 16 B of stats per row
//   backward  reads G and z once and writes dz (24 B per element), plus (row ranges) x 2 cols doubles of partial column sums
// Two shapes, chosen from cols and the access width W (2 doubles per lane where cols, pitches and bases allow, 1 otherwise):
//   wave   cols <= 64 W kNormWaveTrips: a power-of-two group of lanes (at most one wave) owns a row, T <= 4 accesses per lane; a
//          workgroup works on 256 / lanes rows at a time; row sums are an xor butterfly inside the group
//   block  wider rows: the 256 lanes of a workgroup own a row, T = 2 .. 8 (W = 2) or 2 .. 16 (W = 1) accesses per lane; row sums are
//          the butterfly per wave and then the four waves' sums through LDS, added in wave order
// Lane l of a group of L lanes owns the columns (t L + l) W .. + W - 1, t < T: every wave-instruction touches one contiguous segment.
// Nothing here uses atomics, and no order of addition depends on the grid or on timing.
// Accuracy.  The variance is two-pass.  rstd gets one Newton step on an exactly formed residual, and the backward pass takes the stored
// (mu, rstd) as exact and carries the low parts of z - mu, of its product with rstd and (ELU, below 0) of gamma x + beta into the column
// sums: a column sum over few rows is then the rounding of its own terms, not of the normalised values' (the kernels are HBM-bound: the
// extra flops are free).
#pragma once
#include "hnh_gat_norm.h"

namespace {

constexpr int kNormWaveTrips = 4, kNormWaves = kBlock / 64;
// the backward pass's row ranges (a function of rows and cols alone): at most kNormRanges of at least 256 rows where a workgroup works
// on several rows at a time (cols <= kNormNarrow), of at least 16 rows where it owns one row at a time
constexpr int64_t kNormRanges = 1024, kNormNarrow = 512, kNormNarrowRows = 256, kNormWideRows = 16;

__device__ __forceinline__ double norm_act(double y, int act) {
    if (act == HNH_ACT_IDENTITY) return y;
    if (act == HNH_ACT_RELU) return y > 0.0 ? y : 0.0;
    return y >= 0.0 ? y : expm1(y);
}
__device__ __forceinline__ double norm_act_slope(double y, int act) {
    if (act == HNH_ACT_IDENTITY) return 1.0;
    if (act == HNH_ACT_RELU) return y > 0.0 ? 1.0 : 0.0;
    return y >= 0.0 ? 1.0 : exp(y);
}
// ELU's slope below 0, exp(gamma (x + xl) + beta), to about a unit of the last place: y = fma(gamma, x, beta) itself carries up to |y| eps / 2,
// which exp would turn into a relative error of the slope; yl is what y's rounding dropped (p + pl == gamma x, s + es == p + beta, exactly)
__device__ __forceinline__ double norm_elu_slope(double ga, double x, double xl, double be, double y) {
    const double p = ga * x, pl = fma(ga, x, -p);
    const double s = p + be, bb = s - p;
    const double es = (p - (s - bb)) + (be - bb);
    const double yl = ((s - y) + es) + fma(ga, xl, pl);
    const double e = exp(y);
    return fma(e, yl, e);
}

// The sums of a and b over the row's lanes in ONE reduction; every lane of the row ends with the same bits.  BLOCK: `slots` are
// 2 * kNormWaves doubles of LDS that nobody writes again before the workgroup's next barrier.
template <bool BLOCK>
__device__ __forceinline__ void norm_row_sum2(double& a, double& b, int lpr, double* slots) {
    for (int m = (BLOCK ? 32 : lpr >> 1); m >= 1; m >>= 1) {
        a += __shfl_xor(a, m, 64);
        b += __shfl_xor(b, m, 64);
    }
    if constexpr (BLOCK) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            slots[wave] = a;
            slots[kNormWaves + wave] = b;
        }
        __syncthreads();
        a = slots[0];
        b = slots[kNormWaves];
#pragma unroll
        for (int w = 1; w < kNormWaves; w++) {
            a += slots[w];
            b += slots[kNormWaves + w];
        }
    }
}

// (out may be z: neither is __restrict__; a lane reads all of its elements before it writes the first)
template <int W, int T, bool BLOCK>
__global__ __launch_bounds__(kBlock) void layernorm_fwd_kernel(double* out, int64_t ld_out, const double* z, int64_t ld_z, double* __restrict__ stats,
                                                               const double* __restrict__ gamma, const double* __restrict__ beta, int64_t rows, int cols,
                                                               double eps, int act, int lpr_log2) {
    __shared__ double slots[2][2 * kNormWaves];
    const int tid = threadIdx.x;
    const int lpr = BLOCK ? kBlock : 1 << lpr_log2;
    const int lig = BLOCK ? tid : tid & (lpr - 1);
    const int64_t row = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (kBlock >> lpr_log2) + (tid >> lpr_log2);
    if (row >= rows) return;  // (whole groups leave: the butterfly stays inside a group; BLOCK: the grid is the row count)
    const double* zr = z + row * ld_z;
    double* orow = out + row * ld_out;
    double v[T][W];
    double s = 0.0, unused = 0.0;
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (t * lpr + lig) * W;
#pragma unroll
        for (int w = 0; w < W; w++) v[t][w] = 0.0;
        if (c < cols) {  // (W == 2: cols is even)
            if constexpr (W == 2) {
                const double2 a = *reinterpret_cast<const double2*>(zr + c);
                v[t][0] = a.x; v[t][1] = a.y;
            } else {
                v[t][0] = zr[c];
            }
        }
#pragma unroll
        for (int w = 0; w < W; w++) s += v[t][w];
    }
    norm_row_sum2<BLOCK>(s, unused, lpr, slots[0]);
    const double mu = s / (double)cols;
    double q = 0.0;
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (t * lpr + lig) * W;
#pragma unroll
        for (int w = 0; w < W; w++) {
            v[t][w] = c < cols ? v[t][w] - mu : 0.0;  // the deviation, formed before it is squared
            q = fma(v[t][w], v[t][w], q);
        }
    }
    unused = 0.0;
    norm_row_sum2<BLOCK>(q, unused, lpr, slots[1]);
    // 1 / sqrt(var) with one Newton step on the exact residual 1 - var r^2 (tr + tl == var r): rstd is the one number every element of the row and
    // of its gradients is multiplied by, and the backward pass takes it as exact
    const double var = q / (double)cols + eps;
    double rstd = 1.0 / sqrt(var);
    const double tr = var * rstd, tl = fma(var, rstd, -tr);
    rstd = fma(0.5 * rstd, fma(-tr, rstd, 1.0) - tl * rstd, rstd);
    if (lig == 0) {
        stats[2 * row] = mu;
        stats[2 * row + 1] = rstd;
    }
#pragma unroll
    for (int t = 0; t < T; t++) {
        const int c = (t * lpr + lig) * W;
        if (c < cols) {
            double o[W];
#pragma unroll
            for (int w = 0; w < W; w++) o[w] = norm_act(fma(gamma[c + w], v[t][w] * rstd, beta[c + w]), act);
            if constexpr (W == 2) *reinterpret_cast<double2*>(orow + c) = make_double2(o[0], o[1]);
            else orow[c] = o[0];
        }
    }
}

// Workgroup b owns the rows [b per, min((b + 1) per, rows)).  wave shape: group p of the workgroup's 256 / L groups takes the rows
// first + p, first + p + groups, .. in that order, and lane 0's group adds the groups' column sums in group order.  block shape: the
// workgroup takes its rows one after the other.  Either way a column's rows are added in an order that (rows, cols, W) fix.
// (dz may be g: neither is __restrict__; a lane reads all of its elements of a row before it writes the first)
template <int W, int T, bool BLOCK>
__global__ __launch_bounds__(kBlock) void layernorm_bwd_kernel(double* dz, int64_t ld_dz, double* __restrict__ work, const double* g, int64_t ld_g,
                                                               const double* __restrict__ z, int64_t ld_z, const double* __restrict__ stats,
                                                               const double* __restrict__ gamma, const double* __restrict__ beta, int64_t rows, int cols,
                                                               int act, int64_t per, int lpr_log2) {
    constexpr int kLds = BLOCK ? 2 * 2 * kNormWaves : 2 * kBlock * T * W;
    __shared__ double lds[kLds];
    const int tid = threadIdx.x;
    const int lpr = BLOCK ? kBlock : 1 << lpr_log2;
    const int lig = BLOCK ? tid : tid & (lpr - 1);
    const int groups = BLOCK ? 1 : kBlock >> lpr_log2, grp = BLOCK ? 0 : tid >> lpr_log2;
    const int64_t first = (int64_t)blockIdx.x * per;
    const int64_t last = first + per < rows ? first + per : rows;
    double ag[T][W], ab[T][W];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int w = 0; w < W; w++) ag[t][w] = ab[t][w] = 0.0;
    int parity = 0;
    for (int64_t row = first + grp; row < last; row += groups) {  // (BLOCK: the same trip count in every lane, the barriers are uniform)
        const double mu = stats[2 * row], rstd = stats[2 * row + 1];
        const double* gr = g + row * ld_g;
        const double* zr = z + row * ld_z;
        double* dr = dz + row * ld_dz;
        double tv[T][W], xh[T][W];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (t * lpr + lig) * W;
#pragma unroll
            for (int w = 0; w < W; w++) tv[t][w] = xh[t][w] = 0.0;
            if (c < cols) {
                double gv[W], zv[W];
                if constexpr (W == 2) {
                    const double2 a = *reinterpret_cast<const double2*>(gr + c);
                    const double2 b = *reinterpret_cast<const double2*>(zr + c);
                    gv[0] = a.x; gv[1] = a.y;
                    zv[0] = b.x; zv[1] = b.y;
                } else {
                    gv[0] = gr[c];
                    zv[0] = zr[c];
                }
#pragma unroll
                for (int w = 0; w < W; w++) {
                    const double ga = gamma[c + w];
                    // x + xl is the normalised value to about eps^2 given the stats: the difference's rounding error (de) and the
                    // product's (the fma) are kept for the column sum, whose first rows would otherwise carry them whole
                    const double d = zv[w] - mu, bb = d - zv[w];
                    const double de = (zv[w] - (d - bb)) - (mu + bb);
                    const double x = d * rstd;
                    const double xl = fma(d, rstd, -x) + de * rstd;
                    const double be = beta[c + w], y = fma(ga, x, be);  // y is recomputed, not stored: the forward pass's bits, so the same gate
                    const double dy = gv[w] * (act == HNH_ACT_ELU && y < 0.0 ? norm_elu_slope(ga, x, xl, be, y) : norm_act_slope(y, act));
                    ag[t][w] = fma(dy, x, fma(dy, xl, ag[t][w]));
                    ab[t][w] += dy;
                    xh[t][w] = x;
                    tv[t][w] = ga * dy;
                    s1 += tv[t][w];
                    s2 = fma(tv[t][w], x, s2);
                }
            }
        }
        norm_row_sum2<BLOCK>(s1, s2, lpr, lds + parity * 2 * kNormWaves);
        parity ^= 1;  // (BLOCK: the slots of row r are written again for row r + 2, behind the barrier of row r + 1)
        const double m1 = s1 / (double)cols, m2 = s2 / (double)cols;
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (t * lpr + lig) * W;
            if (c < cols) {
                double o[W];
#pragma unroll
                for (int w = 0; w < W; w++) o[w] = rstd * ((tv[t][w] - m1) - xh[t][w] * m2);
                if constexpr (W == 2) *reinterpret_cast<double2*>(dr + c) = make_double2(o[0], o[1]);
                else dr[c] = o[0];
            }
        }
    }
    double* wg = work + (int64_t)blockIdx.x * 2 * cols;
    if constexpr (BLOCK) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            const int c = (t * lpr + lig) * W;
#pragma unroll
            for (int w = 0; w < W; w++)
                if (c + w < cols) {
                    wg[c + w] = ag[t][w];
                    wg[cols + c + w] = ab[t][w];
                }
        }
    } else {
        const int stride = T * W << lpr_log2;  // a group's columns, the lanes' spare ones included; groups * stride == kBlock * T * W
        double* pg = lds + grp * stride;
        double* pb = lds + kBlock * T * W + grp * stride;
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int w = 0; w < W; w++) {
                pg[(t * lpr + lig) * W + w] = ag[t][w];
                pb[(t * lpr + lig) * W + w] = ab[t][w];
            }
        __syncthreads();
        if (grp == 0) {
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int w = 0; w < W; w++) {
                    const int c = (t * lpr + lig) * W + w;
                    if (c < cols) {
                        double sg = lds[c], sb = lds[kBlock * T * W + c];
                        for (int p = 1; p < groups; p++) {
                            sg += lds[p * stride + c];
                            sb += lds[kBlock * T * W + p * stride + c];
                        }
                        wg[c] = sg;
                        wg[cols + c] = sb;
                    }
                }
        }
    }
}

// dgamma = the ranges' first partial rows added front to back, dbeta = their second ones
__global__ __launch_bounds__(kBlock) void layernorm_bwd_finish_kernel(double* __restrict__ dgamma, double* __restrict__ dbeta, const double* __restrict__ work,
                                                                      int64_t cols, int64_t ranges) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= 2 * cols) return;
    double s = work[c];
    for (int64_t q = 1; q < ranges; q++) s += work[q * 2 * cols + c];
    if (c < cols) dgamma[c] = s;
    else dbeta[c - cols] = s;
}

struct NormShape {
    int w = 1, t = 1, lpr_log2 = 0;
    bool block = false;
};
// the shape of a row of `cols` columns at access width w (1 or 2 doubles)
NormShape norm_shape(int64_t cols, int w) {
    NormShape s;
    s.w = w;
    s.block = cols > (int64_t)64 * w * kNormWaveTrips;
    int64_t lanes = kBlock;
    if (!s.block) {  // the smallest power-of-two group that covers the row in one trip, at most one wave
        while (s.lpr_log2 < 6 && ((int64_t)w << s.lpr_log2) < cols) s.lpr_log2++;
        lanes = (int64_t)1 << s.lpr_log2;
    }
    while (lanes * w * s.t < cols) s.t *= 2;
    return s;
}

struct NormPlan {
    int64_t ranges = 1, per = 0;
};
NormPlan norm_bwd_plan(int64_t rows, int64_t cols) {
    NormPlan p;
    const int64_t least = cols <= kNormNarrow ? kNormNarrowRows : kNormWideRows;
    int64_t n = (rows + least - 1) / least;
    if (n > kNormRanges) n = kNormRanges;
    if (n < 1) n = 1;
    p.per = rows > 0 ? (rows + n - 1) / n : 0;
    p.ranges = rows > 0 ? (rows + p.per - 1) / p.per : 1;  // no empty range
    return p;
}

// do the doubles [a, a + na) and [b, b + nb) share a byte?
bool norm_overlap(const double* a, int64_t na, const double* b, int64_t nb) {
    if (a == nullptr || b == nullptr || na <= 0 || nb <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb * sizeof(double) && b0 < a0 + (uintptr_t)na * sizeof(double);
}
int64_t norm_extent(int64_t rows, int64_t ld, int64_t cols) { return rows > 0 ? (rows - 1) * ld + cols : 0; }

// one launch of KERNEL<W, T, BLOCK> at the shape `s`
#define HNH_NORM_LAUNCH(KERNEL, s, grid, st, ...)                                                                                  \
    do {                                                                                                                             \
        const dim3 g_((unsigned)(grid)), b_(kBlock);                                                                                 \
        if (!(s).block && (s).w == 2 && (s).t == 1) hipLaunchKernelGGL((KERNEL<2, 1, false>), g_, b_, 0, st, __VA_ARGS__);           \
        else if (!(s).block && (s).w == 2 && (s).t == 2) hipLaunchKernelGGL((KERNEL<2, 2, false>), g_, b_, 0, st, __VA_ARGS__);      \
        else if (!(s).block && (s).w == 2) hipLaunchKernelGGL((KERNEL<2, 4, false>), g_, b_, 0, st, __VA_ARGS__);                    \
        else if (!(s).block && (s).t == 1) hipLaunchKernelGGL((KERNEL<1, 1, false>), g_, b_, 0, st, __VA_ARGS__);                    \
        else if (!(s).block && (s).t == 2) hipLaunchKernelGGL((KERNEL<1, 2, false>), g_, b_, 0, st, __VA_ARGS__);                    \
        else if (!(s).block) hipLaunchKernelGGL((KERNEL<1, 4, false>), g_, b_, 0, st, __VA_ARGS__);                                  \
        else if ((s).w == 2 && (s).t == 2) hipLaunchKernelGGL((KERNEL<2, 2, true>), g_, b_, 0, st, __VA_ARGS__);                     \
        else if ((s).w == 2 && (s).t == 4) hipLaunchKernelGGL((KERNEL<2, 4, true>), g_, b_, 0, st, __VA_ARGS__);                     \
        else if ((s).w == 2) hipLaunchKernelGGL((KERNEL<2, 8, true>), g_, b_, 0, st, __VA_ARGS__);                                   \
        else if ((s).t == 2) hipLaunchKernelGGL((KERNEL<1, 2, true>), g_, b_, 0, st, __VA_ARGS__);                                   \
        else if ((s).t == 4) hipLaunchKernelGGL((KERNEL<1, 4, true>), g_, b_, 0, st, __VA_ARGS__);                                   \
        else if ((s).t == 8) hipLaunchKernelGGL((KERNEL<1, 8, true>), g_, b_, 0, st, __VA_ARGS__);                                   \
        else hipLaunchKernelGGL((KERNEL<1, 16, true>), g_, b_, 0, st, __VA_ARGS__);                                                  \
    } while (0)

bool norm_known_act(int act) { return act == HNH_ACT_RELU || act == HNH_ACT_ELU || act == HNH_ACT_IDENTITY; }

}  // namespace

extern "C" {

int hnh_layernorm_fwd_f64(hnh_ctx* ctx, double* out, int64_t ld_out, const double* z, int64_t ld_z, double* stats, const double* gamma,
                          const double* beta, int64_t rows, int64_t cols, double eps, int act, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || ld_out < cols || ld_z < cols) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_fwd_f64: bad shape");
    if (!(eps > 0.0) || !(eps < HUGE_VAL)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_fwd_f64: eps must be positive and finite");
    if (!norm_known_act(act))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_fwd_f64: unknown activation " + std::to_string(act) + " (relu = 0, elu = 1, identity = 2)");
    if (cols > HNH_NORM_MAX_COLS)
        return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "hnh_layernorm_fwd_f64: rows of at most " + std::to_string(HNH_NORM_MAX_COLS) + " columns, not " + std::to_string(cols));
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!out || !z || !stats || !gamma || !beta) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_fwd_f64: null pointer");
    const int64_t n_out = norm_extent(rows, ld_out, cols), n_z = norm_extent(rows, ld_z, cols);
    const bool in_place = (const double*)out == z && ld_out == ld_z;
    if ((!in_place && norm_overlap(out, n_out, z, n_z)) || norm_overlap(stats, 2 * rows, out, n_out) || norm_overlap(stats, 2 * rows, z, n_z) ||
        norm_overlap(gamma, cols, out, n_out) || norm_overlap(beta, cols, out, n_out) || norm_overlap(gamma, cols, stats, 2 * rows) ||
        norm_overlap(beta, cols, stats, 2 * rows))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_fwd_f64: an output overlaps an operand (only out == z at the same pitch is allowed)");
    const bool vec = cols % 2 == 0 && ld_out % 2 == 0 && ld_z % 2 == 0 && aligned16(out) && aligned16(z);
    const NormShape s = norm_shape(cols, vec ? 2 : 1);
    const int64_t groups = s.block ? 1 : kBlock >> s.lpr_log2, blocks = (rows + groups - 1) / groups;
    if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "hnh_layernorm_fwd_f64: too many rows for one launch");
    hipStream_t st = ctx->streams[stream];
    HNH_NORM_LAUNCH(layernorm_fwd_kernel, s, blocks, st, out, ld_out, z, ld_z, stats, gamma, beta, rows, (int)cols, eps, act, s.lpr_log2);
    return hnh::check_hip(ctx, hipGetLastError(), "layernorm_fwd_kernel launch");
}

int64_t hnh_layernorm_bwd_workspace(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || cols > HNH_NORM_MAX_COLS) return 0;
    return norm_bwd_plan(rows, cols).ranges * 2 * cols;
}

int hnh_layernorm_bwd_f64(hnh_ctx* ctx, double* dz, int64_t ld_dz, double* dgamma, double* dbeta, const double* G, int64_t ld_g, const double* z,
                          int64_t ld_z, const double* stats, const double* gamma, const double* beta, int64_t rows, int64_t cols, int act,
                          double* work, int64_t work_doubles, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || ld_dz < cols || ld_g < cols || ld_z < cols) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_bwd_f64: bad shape");
    if (!norm_known_act(act))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_bwd_f64: unknown activation " + std::to_string(act) + " (relu = 0, elu = 1, identity = 2)");
    if (cols > HNH_NORM_MAX_COLS)
        return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "hnh_layernorm_bwd_f64: rows of at most " + std::to_string(HNH_NORM_MAX_COLS) + " columns, not " + std::to_string(cols));
    if (cols == 0) return HNH_OK;
    if (!dgamma || !dbeta) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_bwd_f64: null pointer");
    if (norm_overlap(dgamma, cols, dbeta, cols)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_bwd_f64: dgamma overlaps dbeta");
    hipStream_t st = ctx->streams[stream];
    if (rows == 0) {  // empty sums
        HNH_TRY_HIP(ctx, hipMemsetAsync(dgamma, 0, sizeof(double) * (size_t)cols, st));
        HNH_TRY_HIP(ctx, hipMemsetAsync(dbeta, 0, sizeof(double) * (size_t)cols, st));
        return HNH_OK;
    }
    const NormPlan p = norm_bwd_plan(rows, cols);
    const int64_t n_work = p.ranges * 2 * cols;
    if (!dz || !G || !z || !stats || !gamma || !beta || !work || work_doubles < n_work)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_bwd_f64: null pointer or a workspace smaller than hnh_layernorm_bwd_workspace()");
    const int64_t n_dz = norm_extent(rows, ld_dz, cols), n_g = norm_extent(rows, ld_g, cols), n_z = norm_extent(rows, ld_z, cols);
    const bool in_place = (const double*)dz == G && ld_dz == ld_g;
    const double* outs[4] = {dz, dgamma, dbeta, work};
    const int64_t n_outs[4] = {n_dz, cols, cols, n_work};
    const double* ins[5] = {G, z, stats, gamma, beta};
    const int64_t n_ins[5] = {n_g, n_z, 2 * rows, cols, cols};
    bool clash = false;
    for (int a = 0; a < 4; a++) {
        for (int b = a + 1; b < 4; b++) clash = clash || norm_overlap(outs[a], n_outs[a], outs[b], n_outs[b]);
        for (int b = 0; b < 5; b++) clash = clash || (!(a == 0 && b == 0 && in_place) && norm_overlap(outs[a], n_outs[a], ins[b], n_ins[b]));
    }
    if (clash) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_layernorm_bwd_f64: an output overlaps an operand or another output (only dz == G at the same pitch is allowed)");
    const bool vec = cols % 2 == 0 && ld_dz % 2 == 0 && ld_g % 2 == 0 && ld_z % 2 == 0 && aligned16(dz) && aligned16(G) && aligned16(z);
    const NormShape s = norm_shape(cols, vec ? 2 : 1);
    HNH_NORM_LAUNCH(layernorm_bwd_kernel, s, p.ranges, st, dz, ld_dz, work, G, ld_g, z, ld_z, stats, gamma, beta, rows, (int)cols, act, p.per, s.lpr_log2);
    if (int rc = hnh::check_hip(ctx, hipGetLastError(), "layernorm_bwd_kernel launch")) return rc;
    hipLaunchKernelGGL(layernorm_bwd_finish_kernel, dim3((unsigned)((2 * cols + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dgamma, dbeta, work, cols, p.ranges);
    return hnh::check_hip(ctx, hipGetLastError(), "layernorm_bwd_finish_kernel launch");
}

}  // extern "C"
