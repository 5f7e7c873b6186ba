// Dropout for the GAT (include/hnh_attn_dropout.h).  Included at the end of hnh_kernels.hip, after hnh_attn_additive_kernels.hpp: the three
// passes are the DROP instances of attn_add_process and its tag AaPass there, in the shells attn_rows_kernel / attn_segments_kernel (a template
// parameter and `if constexpr`: the plain instances are compiled from the same text and keep their registers), with the parents' dispatch — windows,
// plans, cache panels, hub-row segments, the sequential row-state protocol.  The lane that owns a nonzero of a batch computes its exp AND
// its Philox word; the factor c m_ij goes round with the group broadcast.  Here: the entry points and the elementwise kernels.
#pragma once

namespace {

// M'[r, :] = [A_r (0) | <A_r, a1> <A_r, a2> | id 0], one wave per row (attn_add_scores_kernel plus the id pair)
__global__ __launch_bounds__(kBlock) void attn_drop_scores_kernel(double* __restrict__ M, int64_t ld_m, const double* __restrict__ A, int64_t ld_a,
                                                                  const double* __restrict__ a1, const double* __restrict__ a2, int64_t rows, int f, int fp,
                                                                  int64_t row_id0) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / 64;
    const int lane = threadIdx.x % 64;
    if (row >= rows) return;
    double s = 0.0, t = 0.0;
    for (int c = lane; c < f; c += 64) {
        const double v = A[row * ld_a + c];
        s = fma(v, a1[c], s);
        t = fma(v, a2[c], t);
        M[row * ld_m + c] = v;
    }
    s = group_sum<64>(s);
    t = group_sum<64>(t);
    if (lane == 0) {
        if (fp != f) M[row * ld_m + f] = 0.0;
        M[row * ld_m + fp] = s;
        M[row * ld_m + fp + 1] = t;
        M[row * ld_m + fp + 2] = (double)(row_id0 + row);
        M[row * ld_m + fp + 3] = 0.0;
    }
}

// Q'[r, :] = [dZ_r (0) | s_r lse_r delta_r id_r]
__global__ __launch_bounds__(kBlock) void attn_drop_pack_kernel(double* __restrict__ Q, int64_t ld_q, const double* __restrict__ dZ, int64_t ld_dz,
                                                                const double* __restrict__ M, int64_t ld_m, const double* __restrict__ lse,
                                                                const double* __restrict__ delta, int64_t rows, int f, int fp, int64_t row_id0) {
    const int pw = fp + 4;
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * pw;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / pw;
        const int c = (int)(i % pw);
        double v = 0.0;
        if (c < f) v = dZ[r * ld_dz + c];
        else if (c == fp) v = M[r * ld_m + fp];
        else if (c == fp + 1) v = lse[r];
        else if (c == fp + 2) v = delta[r];
        else if (c == fp + 3) v = (double)(row_id0 + r);
        Q[r * ld_q + c] = v;
    }
}

__global__ __launch_bounds__(kBlock) void feat_drop_kernel(double* dst, int64_t ld_dst, const double* src, int64_t ld_src, int64_t rows, int64_t cols,
                                                           int64_t row_id0, unsigned key0, unsigned key1, unsigned w2, unsigned threshold, double scale) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / cols, c = i % cols;
        const unsigned word = philox_word0((unsigned)(row_id0 + r), (unsigned)c, w2, 1u, key0, key1);
        const double v = src[r * ld_src + c];  // (dst may be src: every entry is read and written by the same thread)
        dst[r * ld_dst + c] = word >= threshold ? scale * v : 0.0;
    }
}

__global__ __launch_bounds__(kBlock) void dropout_words_kernel(unsigned* __restrict__ out, const unsigned* __restrict__ gi, const unsigned* __restrict__ gj,
                                                               int64_t n, unsigned key0, unsigned key1, unsigned w2, unsigned tag) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = philox_word0(gi[i], gj[i], w2, tag, key0, key1);
}

}  // namespace

extern "C" {

int hnh_attn_drop_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, const hnh_attn_drop* drop, unsigned flags,
                            const hnh_csr_window* window, int stream) {
    return attn_add_dispatch<0, true>(ctx, b, args, flags, window, stream, "hnh_attn_drop_fwd_csr_p", drop);
}

int hnh_attn_drop_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, const hnh_attn_drop* drop, unsigned flags,
                            const hnh_csr_window* window, int stream) {
    return attn_add_dispatch<1, true>(ctx, b, args, flags, window, stream, "hnh_attn_drop_row_csr_p", drop);
}

int hnh_attn_drop_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, const hnh_attn_drop* drop, unsigned flags,
                            const hnh_csr_window* window, int stream) {
    return attn_add_dispatch<2, true>(ctx, b, args, flags, window, stream, "hnh_attn_drop_col_csr_p", drop);
}

int hnh_attn_drop_scores_f64(hnh_ctx* ctx, double* M, int64_t ld_m, const double* A, int64_t ld_a, const double* a1, const double* a2,
                             int64_t rows, int f, int64_t row_id0, int stream) {
    HNH_ENTER(ctx, stream);
    if (int rc = check_common(ctx, rows, f, "hnh_attn_drop_scores_f64")) return rc;
    const int fp = f + (f & 1);
    if (ld_m < fp + 4 || ld_m % 2 != 0 || ld_a < f) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_drop_scores_f64: bad pitch");
    if (row_id0 < 0 || row_id0 + rows > 0x100000000LL) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_drop_scores_f64: row ids do not fit 32 bits");
    if (rows == 0) return HNH_OK;
    if (!M || !A || !a1 || !a2 || M == A) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_drop_scores_f64: null or aliased pointer");
    hipLaunchKernelGGL(attn_drop_scores_kernel, dim3((unsigned)((rows * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->streams[stream], M, ld_m, A, ld_a,
                       a1, a2, rows, f, fp, row_id0);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_drop_scores_kernel launch");
}

int hnh_attn_drop_pack_f64(hnh_ctx* ctx, double* Q, int64_t ld_q, const double* dZ, int64_t ld_dz, const double* M, int64_t ld_m,
                           const double* lse, const double* delta, int64_t rows, int f, int64_t row_id0, int stream) {
    HNH_ENTER(ctx, stream);
    if (int rc = check_common(ctx, rows, f, "hnh_attn_drop_pack_f64")) return rc;
    const int fp = f + (f & 1);
    if (ld_q < fp + 4 || ld_q % 2 != 0 || ld_dz < f || ld_m < fp + 2) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_drop_pack_f64: bad pitch");
    if (row_id0 < 0 || row_id0 + rows > 0x100000000LL) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_drop_pack_f64: row ids do not fit 32 bits");
    if (rows == 0) return HNH_OK;
    if (!Q || !dZ || !M || !lse || !delta) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_drop_pack_f64: null pointer");
    hipLaunchKernelGGL(attn_drop_pack_kernel, dim3(ew_grid(rows * (fp + 4))), dim3(kBlock), 0, ctx->streams[stream], Q, ld_q, dZ, ld_dz, M, ld_m, lse, delta,
                       rows, f, fp, row_id0);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_drop_pack_kernel launch");
}

int hnh_feat_drop_f64(hnh_ctx* ctx, double* dst, int64_t ld_dst, const double* src, int64_t ld_src, int64_t rows, int64_t cols,
                      int64_t row_id0, uint64_t seed, uint32_t w2, uint32_t threshold, double scale, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || cols < 0 || ld_dst < cols || ld_src < cols) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_feat_drop_f64: bad shape or pitch");
    if (row_id0 < 0 || row_id0 + rows > 0x100000000LL || cols > 0x100000000LL)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_feat_drop_f64: ids do not fit 32 bits");
    if (rows == 0 || cols == 0) return HNH_OK;
    if (!dst || !src) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_feat_drop_f64: null pointer");
    hipLaunchKernelGGL(feat_drop_kernel, dim3(ew_grid(rows * cols)), dim3(kBlock), 0, ctx->streams[stream], dst, ld_dst, src, ld_src, rows, cols, row_id0,
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), w2, threshold, scale);
    return hnh::check_hip(ctx, hipGetLastError(), "feat_drop_kernel launch");
}

int hnh_dropout_words_u32(hnh_ctx* ctx, uint32_t* out, const uint32_t* gi, const uint32_t* gj, int64_t n, uint64_t seed, uint32_t w2,
                          uint32_t stream_tag, int stream) {
    HNH_ENTER(ctx, stream);
    if (n < 0) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_dropout_words_u32: negative count");
    if (n == 0) return HNH_OK;
    if (!out || !gi || !gj) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_dropout_words_u32: null pointer");
    hipLaunchKernelGGL(dropout_words_kernel, dim3(ew_grid(n)), dim3(kBlock), 0, ctx->streams[stream], out, gi, gj, n, (unsigned)(seed & 0xffffffffu),
                       (unsigned)(seed >> 32), w2, stream_tag);
    return hnh::check_hip(ctx, hipGetLastError(), "dropout_words_kernel launch");
}

}  // extern "C"
