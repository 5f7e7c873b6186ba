// The Gram term and the guarded CG update of implicit-feedback ALS (include/hnh_als_implicit.h).  Included at the end of hnh_grad.hip.
//
// gram_rows_kernel<NJ, MI, WAVES>: Mp = Out + X * G for a tile of rows, the whole output row in one wave's accumulators.  A wave owns
// MI * 16 rows and all RP = 16 NJ columns: MI x NJ accumulators of v_mfma_f64_16x16x4_f64 (fragment maps as in gemm_tn_kernel above:
// A lane l = A[i = l & 15][k = l >> 4], B lane l = B[k = l >> 4][j = l & 15], C register r of lane l = C[(l >> 4) + 4 r][l & 15]).
// Instances: R <= 16, 32, 64: 32 rows per wave, 8 waves; R <= 128: 16 rows per wave, 8 waves; R <= 256: 16 rows per wave, 4 waves
// (the 64 accumulator registers go to the AGPRs, one wave per SIMD).
//   G goes through LDS in K tiles of 16 rows, k-major ([k][n], pitch RP + 4), shared by the workgroup's waves: a workgroup reads G once
//   for its 64 .. 256 rows, from L2 after the first workgroups have pulled it in.  The next tile is fetched into registers under the MFMAs.
//   X does not go through LDS.  The order of the k's inside a K tile is free as long as both operands agree, so lane l loads the FOUR
//   consecutive doubles X[row l & 15][k0 + 4 (l >> 4) ..] (the 16 lanes of a row group read one whole 128-byte line per row) and MFMA
//   step s of the tile multiplies k = k0 + 4 (l >> 4) + s: its B fragment is Gs[4 (l >> 4) + s][16 j + (l & 15)].  Rows four apart in
//   LDS with a pitch of 4 mod 8 doubles put the four row groups of a fragment read on different banks.
//   Epilogue, in the C layout (a row's R values lie in 16 lanes x NJ registers): every row sum adds its NJ registers in order and then
//   the 16 lanes by xor butterflies, a fixed order.  cg mode streams p, r and x past the accumulators (which hold Mp, then the new r)
//   column block by column block, so the update of a 256-wide row needs no more registers than the product; it runs in phases over all of
//   the wave's rows (Mp and <p, Mp>; alpha; r and <r, r>; beta, x and p), each phase a batch of independent loads.
// Traffic in cg mode: Out, X, x, r read and x, r, p written once from HBM (7 matrix passes); p's two re-reads in the epilogue hit the
// lines the product has just pulled in.
#pragma once
#include <string>
#include "hnh_als_implicit.h"

namespace {

constexpr int kGramBK = 16;

// the sum of v over the 16 lanes that share a row of the C layout (lane bits 0 .. 3), in every one of them
__device__ inline double gram_row_sum(double v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int NJ, int MI, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void gram_rows_kernel(double* __restrict__ Out, const double* X, const double* __restrict__ G,
                                                                 int64_t rows, int R, double* __restrict__ rowdot, hnh_gram_cg cg, bool has_cg,
                                                                 bool vec_ok) {
    constexpr int RP = 16 * NJ, LD = RP + 4, kGramWaves = WAVES, kGramThreads = 64 * WAVES;
    constexpr int GPT = (kGramBK * RP + kGramThreads - 1) / kGramThreads;  // doubles of a G tile per thread
    __shared__ double Gs[kGramBK][LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fk = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kGramWaves + wave) * (16 * MI);  // the wave's first row

    d4_t acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[i][j] = (d4_t){0.0, 0.0, 0.0, 0.0};

    double ra[MI][4], rg[GPT];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < MI; i++) {
            const int64_t row = row0 + i * 16 + fr;
            const int k = k0 + 4 * fk;
            if (row < rows && vec_ok && k + 4 <= R) {
                const double2 lo = *reinterpret_cast<const double2*>(X + row * R + k);
                const double2 hi = *reinterpret_cast<const double2*>(X + row * R + k + 2);
                ra[i][0] = lo.x; ra[i][1] = lo.y; ra[i][2] = hi.x; ra[i][3] = hi.y;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) ra[i][q] = (row < rows && k + q < R) ? X[row * R + k + q] : 0.0;
            }
        }
#pragma unroll
        for (int q = 0; q < GPT; q++) {
            const int e = tid + q * kGramThreads, k = k0 + e / RP, n = e % RP;
            rg[q] = (e < kGramBK * RP && k < R && n < R) ? G[(int64_t)k * R + n] : 0.0;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < GPT; q++) {
            const int e = tid + q * kGramThreads;
            if (e < kGramBK * RP) Gs[e / RP][e % RP] = rg[q];
        }
    };

    const int ktiles = (R + kGramBK - 1) / kGramBK;
    fetch(0);
    for (int t = 0; t < ktiles; t++) {
        stage();
        __syncthreads();
        double a[MI][4];
#pragma unroll
        for (int i = 0; i < MI; i++)
#pragma unroll
            for (int q = 0; q < 4; q++) a[i][q] = ra[i][q];
        if (t + 1 < ktiles) fetch((t + 1) * kGramBK);  // in flight during the MFMAs below
#pragma unroll
        for (int s = 0; s < 4; s++) {
            double b[NJ];
#pragma unroll
            for (int j = 0; j < NJ; j++) b[j] = Gs[4 * fk + s][16 * j + fr];
#pragma unroll
            for (int i = 0; i < MI; i++)
#pragma unroll
                for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][s], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();  // the tile's readers are done before the next one is staged
    }

    // ---- the row-wise epilogue: register r of accumulator (i, j) is row row0 + 16 i + fk + 4 r, column 16 j + fr.  In PHASES over all of
    // the wave's rows, each a batch of independent loads (the state's four matrices are told apart with __restrict__: p is only touched
    // through cg.p from here on).
    bool in_row[MI][4];
    int64_t base[MI][4];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = row0 + i * 16 + fk + 4 * r;
            in_row[i][r] = row < rows;  // (uniform over the 16 lanes of the row)
            base[i][r] = row * R;
        }
    // Every load below is UNCONDITIONAL, from a clamped address (element 0 where the lane has no element), and a select drops what it
    // brought: a load inside a branch is waited for inside it, one trip to memory per element instead of one per batch.
    const double* __restrict__ xin = has_cg ? cg.p : X;
    const bool want_dot = has_cg || rowdot != nullptr;
    bool ok[MI][4][NJ];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int j = 0; j < NJ; j++) ok[i][r][j] = in_row[i][r] && 16 * j + fr < R;
#define HNH_GRAM_AT(i, r, j) (ok[i][r][j] ? base[i][r] + 16 * (j) + fr : (int64_t)0)
    double dot[MI][4];
    // phase 1: Mp = acc + Out, and <X, Mp>
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            double o[NJ], xv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; j++) o[j] = Out[HNH_GRAM_AT(i, r, j)];
            if (want_dot) {
#pragma unroll
                for (int j = 0; j < NJ; j++) xv[j] = xin[HNH_GRAM_AT(i, r, j)];
            }
            double d = 0.0;
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const double mp = ok[i][r][j] ? acc[i][j][r] + o[j] : 0.0;
                acc[i][j][r] = mp;
                if (want_dot) d = ok[i][r][j] ? __builtin_fma(xv[j], mp, d) : d;
                if (!has_cg && ok[i][r][j]) Out[base[i][r] + 16 * j + fr] = mp;
            }
            dot[i][r] = d;
        }
    if (!has_cg) {
        if (rowdot != nullptr) {
#pragma unroll
            for (int i = 0; i < MI; i++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double d = gram_row_sum(dot[i][r]);
                    if (in_row[i][r] && fr == 0) rowdot[row0 + i * 16 + fk + 4 * r] = d;
                }
        }
        return;
    }
    double* __restrict__ px = cg.x;
    double* __restrict__ pr = cg.r;
    double* __restrict__ pp = cg.p;
    double* __restrict__ prs = cg.rs;
    // phase 2: the guarded alpha
    double rs[MI][4], alpha[MI][4], sq[MI][4];
    bool live[MI][4];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) rs[i][r] = prs[in_row[i][r] ? row0 + i * 16 + fk + 4 * r : (int64_t)0];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double bdot = gram_row_sum(dot[i][r]);
            live[i][r] = in_row[i][r] && rs[i][r] > 0.0 && bdot > 0.0;
            alpha[i][r] = live[i][r] ? rs[i][r] / bdot : 0.0;
        }
    // phase 3: r -= alpha Mp (the accumulators now hold the new r) and <r, r>
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            double rv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; j++) rv[j] = pr[HNH_GRAM_AT(i, r, j)];
            double q = 0.0;
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                double v = rv[j];
                if (live[i][r]) v = __builtin_fma(-alpha[i][r], acc[i][j][r], v);
                if (live[i][r] && ok[i][r][j]) pr[base[i][r] + 16 * j + fr] = v;
                acc[i][j][r] = v;
                q = ok[i][r][j] ? __builtin_fma(v, v, q) : q;
            }
            sq[i][r] = q;
        }
    // phase 4: x += alpha p, p = r + beta p, rs = <r, r>
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double rsnew = gram_row_sum(sq[i][r]);
            const double beta = live[i][r] ? rsnew / rs[i][r] : 0.0;
            double pv[NJ], xv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                pv[j] = pp[HNH_GRAM_AT(i, r, j)];
                xv[j] = px[HNH_GRAM_AT(i, r, j)];
            }
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                if (live[i][r] && ok[i][r][j]) px[base[i][r] + 16 * j + fr] = __builtin_fma(alpha[i][r], pv[j], xv[j]);
                const double pn = live[i][r] ? __builtin_fma(beta, pv[j], acc[i][j][r]) : acc[i][j][r];
                if (ok[i][r][j]) pp[base[i][r] + 16 * j + fr] = pn;
            }
            if (in_row[i][r] && fr == 0) prs[row0 + i * 16 + fk + 4 * r] = rsnew;
        }
#undef HNH_GRAM_AT
}

template <int NJ, int MI, int WAVES>
int launch_gram_rows(hnh_ctx* ctx, hipStream_t st, double* Out, const double* X, const double* G, int64_t rows, int R, double* rowdot,
                     const hnh_gram_cg* cg, bool vec_ok) {
    const int64_t per_group = (int64_t)WAVES * 16 * MI;
    const int64_t groups = (rows + per_group - 1) / per_group;
    const hnh_gram_cg none = {nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL((gram_rows_kernel<NJ, MI, WAVES>), dim3((unsigned)groups), dim3(64 * WAVES), 0, st, Out, X, G, rows, R, rowdot, cg ? *cg : none,
                       cg != nullptr, vec_ok);
    return hnh::check_hip(ctx, hipGetLastError(), "gram_rows_kernel launch");
}

}  // namespace

extern "C" {

int hnh_gram_rows_f64(hnh_ctx* ctx, double* Out, const double* X, const double* G, int64_t rows, int R, double* rowdot, const hnh_gram_cg* cg,
                      int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || R < 1) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gram_rows_f64: negative rows or R < 1");
    if (R > HNH_GRAM_MAX_R)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gram_rows_f64: R = " + std::to_string(R) + " is wider than HNH_GRAM_MAX_R = " +
                                                   std::to_string(HNH_GRAM_MAX_R) + " (compose hnh_gemm_f64 and the row-wise helpers instead)");
    if ((rows + 63) / 64 > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gram_rows_f64: too many rows for one launch");
    if (rows == 0) return HNH_OK;
    if (!Out || !X || !G) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gram_rows_f64: null pointer");
    if (Out == X) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gram_rows_f64: Out aliases X");
    if (cg != nullptr) {
        if (!cg->x || !cg->r || !cg->p || !cg->rs) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gram_rows_f64: null pointer in hnh_gram_cg");
        if (cg->p != X) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_gram_rows_f64: cg->p must be the call's X");
    }
    hipStream_t st = ctx->streams[stream];
    const bool vec_ok = R % 4 == 0 && aligned16(X);
    if (R <= 16) return launch_gram_rows<1, 2, 8>(ctx, st, Out, X, G, rows, R, rowdot, cg, vec_ok);
    if (R <= 32) return launch_gram_rows<2, 2, 8>(ctx, st, Out, X, G, rows, R, rowdot, cg, vec_ok);
    if (R <= 64) return launch_gram_rows<4, 2, 8>(ctx, st, Out, X, G, rows, R, rowdot, cg, vec_ok);
    if (R <= 128) return launch_gram_rows<8, 1, 8>(ctx, st, Out, X, G, rows, R, rowdot, cg, vec_ok);
    return launch_gram_rows<16, 1, 4>(ctx, st, Out, X, G, rows, R, rowdot, cg, vec_ok);
}

}  // extern "C"
