// Export of the GAT's per-edge attention coefficients (include/hnh_attn_coef.h): values[e] = exp(z_e - lse_i) for every nonzero of a call.
// Included at the end of hnh_kernels.hip, after hnh_attn_v2_kernels.hpp; it uses the neighbours' machinery as it is (AgUnroll, the
// transposed butterfly, philox_word0, plans, Infinity-Cache panels, hnh_attn_dispatch.hpp) and is kept apart from process_row,
// attn_add_process and attn_v2_process so that none of the existing instances changes by a register.
//
//   DOT, GATV2  one group per row: A_i (and a) in registers, column indices through the scalar cache when the group is a wave, U gathered
//               rows per batch in one of two register buffers, z through the butterfly of U reductions; the lane that ends up owning a
//               nonzero takes one exp and stores 8 bytes (U consecutive values per batch)
//   ADDITIVE    another shape: the 32 lanes of a group run over the row's nonzeros, each makes ONE 16-byte gather of [t_j | id_j], adds
//               s_i, takes the exp (and, with the mask, its Philox word) and stores; consecutive lanes store consecutive values
// A row has no state and a value depends on its own operands alone: no hub-row pass, no atomics, no read of `values`, and the same bits
// for every split of a row into windows, groups of windows or panels.
#pragma once
#include "hnh_attn_coef.h"

namespace {

struct AcArgs {  // hnh_attn_coef as the kernels take it
    const double* X;
    const double* a;
    const double* s;
    const double* lse;
    const double* Y;
    double* values;
    int64_t ld_x, ld_y;
    int f;
    double alpha;
};
struct AcDrop {  // hnh_attn_drop as the kernels take it
    unsigned key0, key1, w2, threshold;
    double scale;
    int64_t row_id0;
};

// SCORE: HNH_ATTN_COEF_DOT or HNH_ATTN_COEF_GATV2
template <int SCORE, int LPR, int VEC, int W, bool EXACT>
__device__ __forceinline__ void attn_coef_process(int64_t row, int beg, int end, const int32_t* __restrict__ colidx, const AcArgs& a, int lig) {
    constexpr int U = AgUnroll<0, LPR, VEC, W>::value;
    constexpr int SUB = LPR / U;  // lanes that end up holding the same reduced value
    static_assert(SUB >= 1, "needs U <= LPR");
    constexpr bool V2 = SCORE == HNH_ATTN_COEF_GATV2;
    bool act[VEC];
    unsigned lane_off[VEC];
    // x = the own row of A, av = the head's vector (0 beyond f: such a column adds nothing to z)
    double x[VEC][W], av[V2 ? VEC : 1][W];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        const int c = (v * LPR + lig) * W;
        act[v] = EXACT ? true : (c < a.f);
        lane_off[v] = (unsigned)c * (unsigned)sizeof(double);
#pragma unroll
        for (int w = 0; w < W; w++) {
            x[v][w] = 0.0;
            if constexpr (V2) av[v][w] = 0.0;
        }
        if (act[v]) {
            load_w_stream<W>(x[v], a.X + row * a.ld_x + c);
            if constexpr (V2) load_w_stream<W>(av[v], a.a + c);
        }
    }
    const double lse_i = a.lse[row];
    const double alpha = a.alpha;
    const uint64_t g_base = reinterpret_cast<uint64_t>(a.Y);
    const uint64_t ld_bytes = (uint64_t)a.ld_y * sizeof(double);

    struct Batch {
        double y[U][VEC][W];
    };

    auto load_idx = [&](auto full, int e, int (&c)[U]) {
        constexpr bool FULL = decltype(full)::value;
        if constexpr (LPR == 64) {
#pragma unroll
            for (int u = 0; u < U; u++) c[u] = (FULL || e + u < end) ? colidx[e + u] : -1;
        } else {
            const int my = e + (lig % U);
            const int cv = (FULL || my < end) ? colidx[my] : -1;
#pragma unroll
            for (int u = 0; u < U; u++) c[u] = __shfl(cv, u, LPR);
        }
    };
    auto gather = [&](auto full, const int (&c)[U], Batch& b) {
        constexpr bool FULL = decltype(full)::value;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool live = FULL || c[u] >= 0;
            uint64_t rowp = g_base + (uint64_t)(unsigned)(live ? c[u] : 0) * ld_bytes;
            if constexpr (LPR == 64) {  // wave-uniform: SGPR base + VGPR offset
                const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)rowp);
                const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(rowp >> 32));
                rowp = ((uint64_t)hi << 32) | lo;
            }
#pragma unroll
            for (int v = 0; v < VEC; v++) {
#pragma unroll
                for (int w = 0; w < W; w++) b.y[u][v][w] = 0.0;
                if (live && act[v]) {
                    unsigned off = lane_off[v];
                    if constexpr (LPR == 64) asm volatile("" : "+v"(off));
                    load_w_global<W>(b.y[u][v], rowp, off);
                }
            }
        }
    };
    auto compute = [&](auto full, int e, const Batch& b) {
        constexpr bool FULL = decltype(full)::value;
        double d[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            double sz = 0.0;
#pragma unroll
            for (int v = 0; v < VEC; v++)
#pragma unroll
                for (int w = 0; w < W; w++) {
                    if constexpr (V2) {
                        const double uu = x[v][w] + b.y[u][v][w];
                        sz = fma(av[v][w], uu > 0.0 ? uu : uu * alpha, sz);
                    } else {
                        sz = fma(x[v][w], b.y[u][v][w], sz);
                    }
                }
            d[u] = sz;
        }
        const double r = group_multi_reduce<LPR, U>(d, lig);  // reduction number lig / SUB
        const int umine = lig / SUB;
        const bool have = FULL || e + umine < end;
        const double z = V2 ? r : (r > 0.0 ? r : r * alpha);
        if (have && lig % SUB == 0) store_stream(a.values + e + umine, exp(z - lse_i));
    };
    const BoolTag<true> kFull;
    const BoolTag<false> kMasked;

    int e = beg;
    Batch ba, bb;
    if (e + U <= end) {
        int c0[U], c1[U];
        load_idx(kFull, e, c0);
        gather(kFull, c0, ba);
        for (;;) {
            const bool more = e + 2 * U <= end;
            if (more) {  // the next batch's gathers fly while this one is computed
                load_idx(kFull, e + U, c1);
                gather(kFull, c1, bb);
            }
            __builtin_amdgcn_sched_barrier(0);
            compute(kFull, e, ba);
            __builtin_amdgcn_sched_barrier(0);
            e += U;
            if (!more) break;
            const bool more2 = e + 2 * U <= end;
            if (more2) {
                load_idx(kFull, e + U, c0);
                gather(kFull, c0, ba);
            }
            __builtin_amdgcn_sched_barrier(0);
            compute(kFull, e, bb);
            __builtin_amdgcn_sched_barrier(0);
            e += U;
            if (!more2) break;
        }
    }
    if (e < end) {  // fewer than U nonzeros left: one masked batch
        int c0[U];
        load_idx(kMasked, e, c0);
        gather(kMasked, c0, ba);
        compute(kMasked, e, ba);
    }
}

template <int SCORE, int LPR, int VEC, int W, bool EXACT>
__global__ __launch_bounds__(kBlock) void attn_coef_row_kernel(int64_t rows, const int32_t* __restrict__ beg_ptr, const int32_t* __restrict__ end_ptr,
                                                               const int32_t* __restrict__ colidx, AcArgs a) {
    constexpr int GROUPS = kBlock / LPR;
    const int tid = threadIdx.x;
    const int lig = tid % LPR;
    int64_t row = (int64_t)blockIdx.x * GROUPS + tid / LPR;
    if constexpr (LPR == 64) row = ((int64_t)blockIdx.x * GROUPS) + __builtin_amdgcn_readfirstlane(tid >> 6);
    if (row >= rows) return;
    int beg = beg_ptr[row];
    int end = end_ptr[row];
    if constexpr (LPR == 64) {
        beg = __builtin_amdgcn_readfirstlane(beg);
        end = __builtin_amdgcn_readfirstlane(end);
    }
    if (beg >= end) return;  // nothing of this row in the call
    attn_coef_process<SCORE, LPR, VEC, W, EXACT>(row, beg, end, colidx, a, lig);
}

// ADDITIVE: kCoefLanes lanes per row over its nonzeros of the call; T_j = [t_j | id_j] in one 16-byte load
constexpr int kCoefLanes = 32;
template <bool DROP>
__global__ __launch_bounds__(kBlock) void attn_coef_add_kernel(int64_t rows, const int32_t* __restrict__ beg_ptr, const int32_t* __restrict__ end_ptr,
                                                               const int32_t* __restrict__ colidx, AcArgs a, AcDrop dr) {
    const int tid = threadIdx.x;
    const int lig = tid % kCoefLanes;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kCoefLanes) + tid / kCoefLanes;
    if (row >= rows) return;
    const int beg = beg_ptr[row], end = end_ptr[row];
    if (beg >= end) return;
    const double s_i = a.s[row], lse_i = a.lse[row];
    const uint64_t g_base = reinterpret_cast<uint64_t>(a.Y);
    const uint64_t ld_bytes = (uint64_t)a.ld_y * sizeof(double);
    [[maybe_unused]] const unsigned own_id = (unsigned)(dr.row_id0 + row);
    for (int e = beg + lig; e < end; e += kCoefLanes) {
        double t[2];
        load_w_global<2>(t, g_base + (uint64_t)(unsigned)colidx[e] * ld_bytes, 0u);
        const double z = s_i + t[0];
        double v = exp((z > 0.0 ? z : z * a.alpha) - lse_i);
        if constexpr (DROP) {
            const unsigned word = philox_word0(own_id, (unsigned)(unsigned long long)t[1], dr.w2, 0u, dr.key0, dr.key1);
            v = word >= dr.threshold ? dr.scale * v : 0.0;
        }
        store_stream(a.values + e, v);
    }
}

// s[r] = <A_r, a1>, T[r, :] = [<A_r, a2> | row_id0 + r], one wave per row: the sums of attn_add_scores_kernel in its order
__global__ __launch_bounds__(kBlock) void attn_coef_scores_kernel(double* __restrict__ s_out, double* __restrict__ T, int64_t ld_t, const double* __restrict__ A,
                                                                  int64_t ld_a, const double* __restrict__ a1, const double* __restrict__ a2, int64_t rows, int f,
                                                                  int64_t row_id0) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / 64;
    const int lane = threadIdx.x % 64;
    if (row >= rows) return;
    double s = 0.0, t = 0.0;
    for (int c = lane; c < f; c += 64) {
        const double v = A[row * ld_a + c];
        s = fma(v, a1[c], s);
        t = fma(v, a2[c], t);
    }
    s = group_sum<64>(s);
    t = group_sum<64>(t);
    if (lane == 0) {
        s_out[row] = s;
        T[row * ld_t] = t;
        T[row * ld_t + 1] = (double)(row_id0 + row);
    }
}

template <int SCORE, int LPR, int VEC, int W, bool EXACT>
int attn_coef_launch(hnh_ctx* ctx, hipStream_t st, const LongCtl& lc, int64_t rows, const int32_t* beg_ptr, const int32_t* end_ptr, const int32_t* colidx,
                     const AcArgs& a) {
    constexpr int GROUPS = kBlock / LPR;
    const int64_t blocks = (rows + GROUPS - 1) / GROUPS;
    if (blocks <= 0) return HNH_OK;
    if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "too many rows for one launch");
    const size_t lds_pad = lc.lds_pad <= 48 * 1024 ? lc.lds_pad : 0;
    hipLaunchKernelGGL((attn_coef_row_kernel<SCORE, LPR, VEC, W, EXACT>), dim3((unsigned)blocks), dim3(kBlock), lds_pad, st, rows, beg_ptr, end_ptr, colidx, a);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_coef_row_kernel launch");
}

}  // namespace

extern "C" {

int hnh_attn_coef_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, double* values, const hnh_attn_coef* g, const hnh_attn_drop* drop, unsigned flags,
                        const hnh_csr_window* win, int stream) {
    const char* who = "hnh_attn_coef_csr_p";
    HNH_ENTER(ctx, stream);
    if (!b || !g) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null block or arguments");
    if (int rc = check_common(ctx, b->rows, g->f, who)) return rc;
    if (flags) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": unknown flag");
    if (g->score != HNH_ATTN_COEF_DOT && g->score != HNH_ATTN_COEF_ADDITIVE && g->score != HNH_ATTN_COEF_GATV2)
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": unknown score " + std::to_string(g->score));
    if (g->f > HNH_ATTN_COEF_MAX_F)
        return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, std::string(who) + ": head width " + std::to_string(g->f) + " beyond the limit of " +
                                                       std::to_string(HNH_ATTN_COEF_MAX_F) + " (HNH_ATTN_COEF_MAX_F)");
    const bool additive = g->score == HNH_ATTN_COEF_ADDITIVE;
    if (drop != nullptr && !additive)
        return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, std::string(who) + ": the mask belongs to score additive (include/hnh_attn_dropout.h)");
    if (b->rows == 0) return HNH_OK;
    if (b->rowptr == nullptr) {  // a block without nonzeros: nothing to store
        if (b->nnz > 0) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null rowptr");
        return HNH_OK;
    }
    if (!b->col_idx || !values || !g->lse || !g->Y) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null pointer");
    const int f = g->f;
    AcArgs a = {};
    a.X = g->X; a.a = g->a; a.s = g->s; a.lse = g->lse; a.Y = g->Y; a.values = values;
    a.ld_x = g->ld_x; a.ld_y = g->ld_y; a.f = f; a.alpha = g->leaky_alpha;
    if ((const double*)values == g->Y || (const double*)values == g->lse) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": values aliases an input");
    hipStream_t st = ctx->streams[stream];

    if (additive) {
        if (!g->s) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null s");
        if (g->ld_y < HNH_ATTN_COEF_PAIR_WIDTH || g->ld_y % 2 != 0 || !aligned16(g->Y))
            return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": the packed pair needs an even pitch of at least 2 and a 16-byte aligned base");
        AcDrop dr = {};
        if (drop != nullptr) {
            if (drop->row_id0 < 0 || drop->row_id0 + b->rows > 0x100000000LL)
                return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": the block's global row ids do not fit 32 bits");
            dr.key0 = (unsigned)(drop->seed & 0xffffffffu);
            dr.key1 = (unsigned)(drop->seed >> 32);
            dr.w2 = drop->w2;
            dr.threshold = drop->threshold;
            dr.scale = drop->scale;
            dr.row_id0 = drop->row_id0;
        }
        auto launch = [&](const LongCtl&, const int32_t* beg_ptr, const int32_t* end_ptr, unsigned, bool) {
            constexpr int GROUPS = kBlock / kCoefLanes;
            const int64_t blocks = (b->rows + GROUPS - 1) / GROUPS;
            if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "too many rows for one launch");
            if (drop != nullptr)
                hipLaunchKernelGGL(attn_coef_add_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, b->rows, beg_ptr, end_ptr, b->col_idx, a, dr);
            else
                hipLaunchKernelGGL(attn_coef_add_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, b->rows, beg_ptr, end_ptr, b->col_idx, a, dr);
            return hnh::check_hip(ctx, hipGetLastError(), "attn_coef_add_kernel launch");
        };
        // (pitch 0: no hub-row pass; the gathered operand is 2 doubles wide)
        return attn_dispatch_tail(ctx, st, stream, b, win, HNH_ATTN_COEF_PAIR_WIDTH, true, 0, HNH_ATTN_COEF_PAIR_WIDTH, 0u, who, launch);
    }

    const bool v2 = g->score == HNH_ATTN_COEF_GATV2;
    if (!g->X || (v2 && !g->a)) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null pointer");
    if (g->ld_x < f || g->ld_y < f) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": a pitch is narrower than f");
    const bool w2 = f % 2 == 0 && aligned16(g->X) && g->ld_x % 2 == 0 && aligned16(g->Y) && g->ld_y % 2 == 0 && (!v2 || aligned16(g->a));
    auto launch = [&](const LongCtl& lc, const int32_t* beg_ptr, const int32_t* end_ptr, unsigned, bool) {
        return attn_launch_shape(f, w2, [&](auto l, auto v, auto w, auto ex) {
            if (v2)
                return attn_coef_launch<HNH_ATTN_COEF_GATV2, decltype(l)::value, decltype(v)::value, decltype(w)::value, decltype(ex)::value>(
                    ctx, st, lc, b->rows, beg_ptr, end_ptr, b->col_idx, a);
            return attn_coef_launch<HNH_ATTN_COEF_DOT, decltype(l)::value, decltype(v)::value, decltype(w)::value, decltype(ex)::value>(
                ctx, st, lc, b->rows, beg_ptr, end_ptr, b->col_idx, a);
        });
    };
    // (pitch 0: hub rows are walked by their group like every other row)
    return attn_dispatch_tail(ctx, st, stream, b, win, f, w2, 0, f, 0u, who, launch);
}

int hnh_attn_coef_scores_f64(hnh_ctx* ctx, double* s, double* T, int64_t ld_t, const double* A, int64_t ld_a, const double* a1, const double* a2,
                             int64_t rows, int f, int64_t row_id0, int stream) {
    HNH_ENTER(ctx, stream);
    if (int rc = check_common(ctx, rows, f, "hnh_attn_coef_scores_f64")) return rc;
    if (ld_t < HNH_ATTN_COEF_PAIR_WIDTH || ld_t % 2 != 0 || ld_a < f) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_coef_scores_f64: bad pitch");
    if (row_id0 < 0 || row_id0 + rows > (1LL << 53)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_coef_scores_f64: row ids beyond 2^53");
    if (rows == 0) return HNH_OK;
    if (!s || !T || !A || !a1 || !a2 || s == A || T == A || s == T || !aligned16(T))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_coef_scores_f64: null, aliased or misaligned pointer");
    hipLaunchKernelGGL(attn_coef_scores_kernel, dim3((unsigned)((rows * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->streams[stream], s, T, ld_t, A,
                       ld_a, a1, a2, rows, f, row_id0);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_coef_scores_kernel launch");
}

}  // extern "C"
