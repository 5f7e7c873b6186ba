// The fused backward pass of the GAT's attention (include/hnh_attn_grad.h): two sibling templates of the row kernel.  Included at the
// end of hnh_kernels.hip — same translation unit, because the passes share the row kernels' machinery (transposed butterfly, hub-row
// work lists and partial-row scratch, structure plans, Infinity-Cache panels) — and kept apart from process_row so that none of the
// existing instances changes by a register.
//
//   AgPass<0, ..>   ROW pass over S:      x = A_i, z = dZ_i, lse_i, delta_i in registers; gathers y = A_j (f wide)
//                   e = <x, y>, da = <z, y>, gate, acc += de y
//   AgPass<1, ..>   COLUMN pass over S^T: x = A_j in registers; gathers the packed P_i = [A_i | dZ_i | lse_i delta_i]
//                   e = <x, ya>, da = <x, yz>, gate with the gathered row's scalars, acc += a yz + de ya
// Lane layout as in process_row: a group of LPR lanes owns a sparse row, lane l holds elements (v LPR + l) W .. + W of a dense row for
// v < VEC.  U nonzeros are gathered per batch into one of two register buffers (the next batch's gathers fly while this one is
// computed); their 2 U dot products go through ONE transposed butterfly of 2 U reductions, after which the lower half of the group
// holds the e's and the upper half the da's of the same nonzeros — one more exchange across the halves gives every lane both.
// The gate is evaluated per lane (softmax: one exp per nonzero), the weights are handed round with group broadcasts as in kFused.
// U is chosen so that a batch is at most 16 gathered doubles per lane: 32 doubles (64 VGPRs) of gather buffers in every instance.
#pragma once
#include "hnh_attn_dispatch.hpp"

namespace {

struct AgArgs {  // hnh_attn_grad as the kernels take it
    const double* X;
    const double* dZ;
    const double* lse;
    const double* delta;
    const double* Y;
    double* Out;
    int64_t ld_x, ld_dz, ld_y, ld_out;
    int f, fp;  // fp = f rounded up to even: column of the dZ half of a packed row (the two scalars sit at 2 fp)
    int softmax;
    double alpha;
};

template <int PASS, int LPR, int VEC, int W>
struct AgUnroll {
    static constexpr int per_nz = (PASS == 1 ? 2 : 1) * VEC * W;  // gathered doubles per lane and nonzero
    static constexpr int by_regs = 16 / per_nz < 1 ? 1 : (16 / per_nz > 8 ? 8 : 16 / per_nz);
    static constexpr int value = 2 * by_regs <= LPR ? by_regs : LPR / 2;
};

template <int PASS, int LPR, int VEC, int W, bool EXACT>
__device__ __forceinline__ void attn_grad_process(int64_t row, int beg, int end, const int32_t* __restrict__ colidx, const AgArgs& a,
                                                  unsigned flags, int lig, double* part_row) {
    constexpr int U = AgUnroll<PASS, LPR, VEC, W>::value;
    constexpr int H = PASS == 1 ? 2 : 1;  // halves of a gathered row
    constexpr int SUB = LPR / (2 * U);    // lanes that end up holding the same reduced value
    static_assert(SUB >= 1, "needs 2 U <= LPR");
    bool act[VEC];
    int coff[VEC];
    unsigned lane_off[VEC];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        const int c = (v * LPR + lig) * W;
        act[v] = EXACT ? true : (c < a.f);
        coff[v] = c;
        lane_off[v] = (unsigned)c * (unsigned)sizeof(double);
    }
    const bool softmax = a.softmax != 0;

    double x[VEC][W], z[PASS == 0 ? VEC : 1][W], acc[VEC][W];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
#pragma unroll
        for (int w = 0; w < W; w++) {
            x[v][w] = 0.0;
            acc[v][w] = 0.0;
            if constexpr (PASS == 0) z[v][w] = 0.0;
        }
        if (act[v]) {
            load_w_stream<W>(x[v], a.X + row * a.ld_x + coff[v]);
            if constexpr (PASS == 0) load_w_stream<W>(z[v], a.dZ + row * a.ld_dz + coff[v]);
            if (part_row == nullptr && !(flags & HNH_FUSED_OUT_OVERWRITE)) load_w_stream<W>(acc[v], a.Out + row * a.ld_out + coff[v]);
        }
    }
    double lse_i = 0.0, delta_i = 0.0;  // row pass: the own row's scalars
    if constexpr (PASS == 0) {
        if (softmax) {
            lse_i = a.lse[row];
            delta_i = a.delta[row];
        }
    }
    const uint64_t g_base = reinterpret_cast<uint64_t>(a.Y);
    const uint64_t ld_bytes = (uint64_t)a.ld_y * sizeof(double);
    const unsigned half_bytes = (unsigned)a.fp * (unsigned)sizeof(double);

    struct Batch {
        double y[U][H][VEC][W];
        double sc[PASS == 1 ? U : 1][2];  // column pass, softmax: lse and delta of the gathered rows
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
            if constexpr (LPR == 64) {  // wave-uniform: SGPR base + VGPR offset, and the two scalars through the scalar cache
                const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)rowp);
                const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(rowp >> 32));
                rowp = ((uint64_t)hi << 32) | lo;
            }
#pragma unroll
            for (int h = 0; h < H; h++)
#pragma unroll
                for (int v = 0; v < VEC; v++) {
#pragma unroll
                    for (int w = 0; w < W; w++) b.y[u][h][v][w] = 0.0;
                    if (live && act[v]) {
                        unsigned off = lane_off[v] + (h ? half_bytes : 0u);
                        if constexpr (LPR == 64) asm volatile("" : "+v"(off));
                        load_w_global<W>(b.y[u][h][v], rowp, off);
                    }
                }
            if constexpr (PASS == 1) {
                b.sc[u][0] = 0.0;
                b.sc[u][1] = 0.0;
                if (softmax && live) {
                    load_w_global<2>(b.sc[u], rowp, 2u * half_bytes);  // (16-byte aligned: an even pitch, 2 fp even)
                }
            }
        }
    };
    auto compute = [&](auto full, int e, const Batch& b) {
        constexpr bool FULL = decltype(full)::value;
        double d[2 * U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            double se = 0.0, sd = 0.0;
#pragma unroll
            for (int v = 0; v < VEC; v++)
#pragma unroll
                for (int w = 0; w < W; w++) {
                    if constexpr (PASS == 0) {
                        se = fma(x[v][w], b.y[u][0][v][w], se);
                        sd = fma(z[v][w], b.y[u][0][v][w], sd);
                    } else {
                        se = fma(x[v][w], b.y[u][0][v][w], se);
                        sd = fma(x[v][w], b.y[u][H - 1][v][w], sd);
                    }
                }
            d[u] = se;
            d[U + u] = sd;
        }
        // reduction number lig / SUB: the lower half of the group ends up with the e's, the upper half with the da's
        const double r = group_multi_reduce<LPR, 2 * U>(d, lig);
        const double o = shfl_xor_f64(r, LPR / 2);
        const bool lower = lig < LPR / 2;
        const double ev = lower ? r : o, da = lower ? o : r;
        const int umine = (lig / SUB) % U;
        const bool have = FULL || e + umine < end;
        double l = lse_i, dl = delta_i;
        if constexpr (PASS == 1) {
#pragma unroll
            for (int u = 0; u < U; u++)
                if (u == umine) {
                    l = b.sc[u][0];
                    dl = b.sc[u][1];
                }
        }
        const double slope = ev > 0.0 ? 1.0 : a.alpha;
        const double s = ev * slope;
        double wa, wde;
        if (softmax) {
            wa = exp(s - l);
            wde = wa * (da - dl) * slope;
        } else {
            wa = s;
            wde = da * slope;
        }
        if (!have) {
            wa = 0.0;
            wde = 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const double du = group_bcast<LPR>(wde, u * SUB);
            if constexpr (PASS == 1) {
                const double au = group_bcast<LPR>(wa, u * SUB);
#pragma unroll
                for (int v = 0; v < VEC; v++)
#pragma unroll
                    for (int w = 0; w < W; w++) acc[v][w] = fma(du, b.y[u][0][v][w], fma(au, b.y[u][H - 1][v][w], acc[v][w]));
            } else {
#pragma unroll
                for (int v = 0; v < VEC; v++)
#pragma unroll
                    for (int w = 0; w < W; w++) acc[v][w] = fma(du, b.y[u][0][v][w], acc[v][w]);
            }
        }
        // pin the accumulation here (as process_row does): sunk to the end of the trip it would keep both gather buffers alive
#pragma unroll
        for (int v = 0; v < VEC; v++)
#pragma unroll
            for (int w = 0; w < W; w++) asm volatile("" : "+v"(acc[v][w]));
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

#pragma unroll
    for (int v = 0; v < VEC; v++) {
        if (!act[v]) continue;
        if (part_row != nullptr) store_w_stream<W>(part_row + coff[v], acc[v]);  // a hub row's segment: added up in order afterwards
        else store_w_stream<W>(a.Out + row * a.ld_out + coff[v], acc[v]);
    }
}

// the instance's name for the shells of hnh_attn_dispatch.hpp (attn_rows_kernel, attn_segments_kernel)
template <int PASS, int LPR, int VEC, int W, bool EXACT>
struct AgPass {
    using Args = AgArgs;
    static constexpr int lpr = LPR;
    static __device__ __forceinline__ void run(int64_t row, int beg, int end, const int32_t* __restrict__ colidx, const AgArgs& a, unsigned flags, int lig,
                                               double* part_row) {
        attn_grad_process<PASS, LPR, VEC, W, EXACT>(row, beg, end, colidx, a, flags, lig, part_row);
    }
};

// P[r, :] = [A_r (0) | dZ_r (0) | lse_r delta_r], the layout of include/hnh_attn_grad.h
__global__ __launch_bounds__(kBlock) void attn_grad_pack_kernel(double* __restrict__ P, int64_t ld_p, const double* __restrict__ A, int64_t ld_a,
                                                                const double* __restrict__ dZ, int64_t ld_dz, const double* __restrict__ lse,
                                                                const double* __restrict__ delta, int64_t rows, int f, int fp, int pw) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * pw;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / pw;
        const int c = (int)(i % pw);
        double v = 0.0;
        if (c < f) v = A[r * ld_a + c];
        else if (c >= fp && c < fp + f) v = dZ[r * ld_dz + (c - fp)];
        else if (c == 2 * fp) v = lse[r];
        else if (c == 2 * fp + 1) v = delta[r];
        P[r * ld_p + c] = v;
    }
}

template <int PASS>
int attn_grad_dispatch(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_grad* g, unsigned flags, const hnh_csr_window* win, int stream,
                       const char* who) {
    HNH_ENTER(ctx, stream);
    if (int rc = attn_dispatch_head(ctx, b, g != nullptr, g ? g->f : 0, HNH_ATTN_GRAD_MAX_F, "HNH_ATTN_GRAD_MAX_F", false, flags, win, who)) return rc;
    if (b->rows == 0) return HNH_OK;
    const int f = g->f, fp = f + (f & 1);
    const bool softmax = PASS == 0 ? (g->lse != nullptr) : (g->softmax != 0);
    if (!g->Out || g->ld_out < f) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad output");
    hipStream_t st = ctx->streams[stream];
    const int64_t pitch = f;  // a segment's partial result: its row
    AttnSums sums;
    sums.add(0, g->Out, g->ld_out, f);
    if (b->rowptr == nullptr) return attn_dispatch_no_nonzeros(ctx, st, b, flags, nullptr, sums, who);
    if (!b->col_idx || !g->X || !g->Y) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null pointer");
    if (g->ld_x < f) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": ld_x is narrower than f");
    if (g->X == g->Out || g->Y == g->Out) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": Out aliases an input");
    bool w2 = f % 2 == 0 && aligned16(g->X) && g->ld_x % 2 == 0 && aligned16(g->Y) && g->ld_y % 2 == 0 && aligned16(g->Out) && g->ld_out % 2 == 0;
    if (PASS == 0) {
        if (!g->dZ || g->ld_dz < f || g->ld_y < f) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad dZ or gathered operand");
        if ((g->lse == nullptr) != (g->delta == nullptr)) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": lse and delta go together");
        if (g->dZ == g->Out) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": Out aliases an input");
        w2 = w2 && aligned16(g->dZ) && g->ld_dz % 2 == 0;
    } else {
        // the packed operand (hnh_attn_grad.h): an even pitch and a 16-byte aligned base, whatever f is
        if (g->ld_y < HNH_ATTN_GRAD_PACKED_WIDTH(f, softmax) || g->ld_y % 2 != 0 || !aligned16(g->Y))
            return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": the packed operand needs an even pitch of at least " +
                                                       std::to_string(HNH_ATTN_GRAD_PACKED_WIDTH(f, softmax)) + " and a 16-byte aligned base");
    }
    AgArgs a;
    a.X = g->X; a.dZ = g->dZ; a.lse = g->lse; a.delta = g->delta; a.Y = g->Y; a.Out = g->Out;
    a.ld_x = g->ld_x; a.ld_dz = g->ld_dz; a.ld_y = g->ld_y; a.ld_out = g->ld_out;
    a.f = f; a.fp = fp; a.softmax = softmax ? 1 : 0; a.alpha = g->leaky_alpha;

    const int gather_w = PASS == 1 ? HNH_ATTN_GRAD_PACKED_WIDTH(f, softmax) : f;
    auto launch = [&](const LongCtl& lc, const int32_t* beg_ptr, const int32_t* end_ptr, unsigned fl, bool run_long) {
        return attn_launch_shape(f, w2, [&](auto l, auto v, auto w, auto ex) {
            return attn_launch<AgPass<PASS, decltype(l)::value, decltype(v)::value, decltype(w)::value, decltype(ex)::value>, false, true>(
                ctx, st, lc, b->rows, b->rowptr, beg_ptr, end_ptr, b->col_idx, a, fl, run_long, pitch, sums);
        });
    };
    return attn_dispatch_tail(ctx, st, stream, b, win, f, w2, pitch, gather_w, flags, who, launch);
}

}  // namespace

extern "C" {

int hnh_attn_grad_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_grad* args, unsigned flags, const hnh_csr_window* window,
                            int stream) {
    return attn_grad_dispatch<0>(ctx, b, args, flags, window, stream, "hnh_attn_grad_row_csr_p");
}

int hnh_attn_grad_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_grad* args, unsigned flags, const hnh_csr_window* window,
                            int stream) {
    return attn_grad_dispatch<1>(ctx, b, args, flags, window, stream, "hnh_attn_grad_col_csr_p");
}

int hnh_attn_grad_pack_f64(hnh_ctx* ctx, double* P, int64_t ld_p, const double* A, int64_t ld_a, const double* dZ, int64_t ld_dz,
                           const double* lse, const double* delta, int64_t rows, int f, int stream) {
    HNH_ENTER(ctx, stream);
    if (int rc = check_common(ctx, rows, f, "hnh_attn_grad_pack_f64")) return rc;
    if ((lse == nullptr) != (delta == nullptr)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_grad_pack_f64: lse and delta go together");
    const int fp = f + (f & 1), pw = HNH_ATTN_GRAD_PACKED_WIDTH(f, lse != nullptr);
    if (ld_p < pw || ld_p % 2 != 0 || ld_a < f || ld_dz < f) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_grad_pack_f64: bad pitch");
    if (rows == 0) return HNH_OK;
    if (!P || !A || !dZ) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_grad_pack_f64: null pointer");
    hipLaunchKernelGGL(attn_grad_pack_kernel, dim3(ew_grid(rows * pw)), dim3(kBlock), 0, ctx->streams[stream], P, ld_p, A, ld_a, dZ, ld_dz, lse, delta,
                       rows, f, fp, pw);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_grad_pack_kernel launch");
}

}  // extern "C"
