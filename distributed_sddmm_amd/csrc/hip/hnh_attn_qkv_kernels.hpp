// Query/key/value attention scores of the GAT (include/hnh_attn_qkv.h): three sibling templates of the row kernel and no dense pass.
// Included at the end of hnh_kernels.hip, after hnh_attn_v2_kernels.hpp, whose neighbours' machinery they use as it is (AgUnroll; from
// hnh_attn_dispatch.hpp the row and segment kernels, the hub-row segment scheme and the dispatcher's head and tail) next to the row
// kernels' transposed butterfly and group broadcast; kept apart from process_row, attn_grad_process, attn_add_process and attn_v2_process
// so that none of the existing instances changes by a register.
//
//   PASS 0  forward over S:        Q_i and the row's softmax state in registers; gathers [K_j | V_j]; s = scale <Q_i, K_j> through a
//                                  butterfly of U reductions, the online-softmax step of kFusedSoftmax, acc = acc f + p V_j
//   PASS 1  backward row pass:     Q_i, dZ_i, lse_i, delta_i in registers; gathers [K_j | V_j]; <Q_i, K_j> and <dZ_i, V_j> through ONE
//                                  butterfly of 2 U reductions, the gate per lane (one exp per nonzero), acc += g K_j  (dQ)
//   PASS 2  backward column pass:  K_j, V_j in registers; gathers the packed P_i = [Q_i | dZ_i | lse_i delta_i] (hnh_attn_grad.h);
//                                  <K_j, Q_i> and <V_j, dZ_i> through one butterfly, the gate with the gathered row's scalars,
//                                  acc += g Q_i (dK) and acc2 += p dZ_i (dV): two accumulators per row, stored to two outputs
// Every gathered row has two halves, so U is that of attn_grad_process's column pass: U nonzeros per batch in one of two register buffers
// (the next batch's gathers fly while this one is computed), at most 16 gathered doubles per lane and batch (f = 256: U = 2).
// The BIAS instances (include/hnh_attn_edge.h) are the same three passes with a per-nonzero addend on the score, and the DBIAS instances
// (include/hnh_attn_edge_grad.h) the two biased backward passes with one more store per nonzero, dL/db_e: see attn_qkv_process.
#pragma once

namespace {

struct AqArgs {  // hnh_attn_qkv as the kernels take it
    const double* X;
    const double* X2;
    const double* dZ;
    const double* delta;
    const double* Y;
    double* lse;
    double* Out;
    double* Out2;
    double* row_max;
    double* row_sum;
    double* relu_dst;
    double* values;
    int64_t ld_x, ld_x2, ld_dz, ld_y, ld_out, ld_out2, relu_ld;
    int f, fp;  // fp = f rounded up to even: column of the second half of a packed row (the two scalars sit at 2 fp)
    double scale;
};

// ... and with the per-edge bias of include/hnh_attn_edge.h: a type of its own, so that the plain instances' kernel arguments stay as they are
struct AqBiasArgs : AqArgs {
    const double* bias;  // bias[e] of nonzero e, in the block's numbering (where values[e] goes)
};

// ... and with the bias's gradient of include/hnh_attn_edge_grad.h, again a type of its own: the BIAS instances' arguments stay as they are
struct AqBiasGradArgs : AqBiasArgs {
    double* dbias;   // dbias[e] of nonzero e, addressed like bias[e]
    int accumulate;  // 0: dbias[e] = p_e (<dZ_i, V_j> - delta_i); otherwise dbias[e] += that (an earlier head's value)
};

template <bool BIAS, bool DBIAS>
using AqArgsOf = std::conditional_t<DBIAS, AqBiasGradArgs, std::conditional_t<BIAS, AqBiasArgs, AqArgs>>;

// BIAS (include/hnh_attn_edge.h): s_e = scale <Q_i, K_j> + bias[e].  The lane that owns nonzero e's score after the butterfly loads bias[e]
// with the batch's column indices, ahead of the gathers, into the batch's buffer (one vector load of 8 bytes per lane: the lanes of a group
// read U consecutive doubles of one line; it works at every LPR, where loads through the scalar cache would need a wave-uniform row), and
// adds it before the online-softmax step (forward) or to the exponent scale qk - lse before the exp (row and column pass).
// DBIAS (include/hnh_attn_edge_grad.h; backward passes with BIAS): after the butterfly every lane of a nonzero's SUB lanes, in both halves of
// the group, holds wp (da - dl) = dL/db_e of this head; one of them (the first of the lower half, as the forward pass stores values[e])
// stores it to dbias[e], or adds it to what is there.  Every nonzero belongs to one (launch, segment): no partial rows, no atomics.
template <int PASS, int LPR, int VEC, int W, bool EXACT, bool BIAS = false, bool DBIAS = false>
__device__ __forceinline__ void attn_qkv_process(int64_t row, int beg, int end, const int32_t* __restrict__ colidx, const AqArgsOf<BIAS, DBIAS>& a,
                                                 unsigned flags, int lig, double* part_row) {
    static_assert(!DBIAS || (BIAS && PASS != 0), "the bias's gradient belongs to the biased backward passes");
    constexpr int U = AgUnroll<1, LPR, VEC, W>::value;  // (two halves per gathered row in every pass)
    constexpr int NR = PASS == 0 ? U : 2 * U;           // reductions of a batch's butterfly
    constexpr int SUB = LPR / NR;                       // lanes that end up holding the same reduced value
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
    const bool fresh = part_row != nullptr || (flags & HNH_FUSED_OUT_OVERWRITE);

    // x = the own row of Q (forward, row pass) or K (column pass), z = dZ_i (row pass) or the own row of V (column pass),
    // acc = the softmax accumulator / dQ / dK, acc2 = dV (column pass)
    double x[VEC][W], z[PASS != 0 ? VEC : 1][W], acc[VEC][W], acc2[PASS == 2 ? VEC : 1][W];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
#pragma unroll
        for (int w = 0; w < W; w++) {
            x[v][w] = 0.0;
            acc[v][w] = 0.0;
            if constexpr (PASS != 0) z[v][w] = 0.0;
            if constexpr (PASS == 2) acc2[v][w] = 0.0;
        }
        if (act[v]) {
            load_w_stream<W>(x[v], a.X + row * a.ld_x + coff[v]);
            if constexpr (PASS == 1) load_w_stream<W>(z[v], a.dZ + row * a.ld_dz + coff[v]);
            if constexpr (PASS == 2) load_w_stream<W>(z[v], a.X2 + row * a.ld_x2 + coff[v]);
            if (!fresh) {
                load_w_stream<W>(acc[v], a.Out + row * a.ld_out + coff[v]);
                if constexpr (PASS == 2) load_w_stream<W>(acc2[v], a.Out2 + row * a.ld_out2 + coff[v]);
            }
        }
    }
    double lse_i = 0.0, delta_i = 0.0;  // row pass: the own row's scalars
    if constexpr (PASS == 1) {
        lse_i = a.lse[row];
        delta_i = a.delta[row];
    }
    double m_run = -__builtin_inf(), l_run = 0.0;  // forward: the row's running max and sum (hnh_attention.h)
    if constexpr (PASS == 0) {
        if (!fresh) {
            m_run = a.row_max[row];
            l_run = a.row_sum[row];
        }
    }
    const double scale = a.scale;
    const uint64_t g_base = reinterpret_cast<uint64_t>(a.Y);
    const uint64_t ld_bytes = (uint64_t)a.ld_y * sizeof(double);
    const unsigned half_bytes = (unsigned)a.fp * (unsigned)sizeof(double);

    struct Batch {
        double y[U][2][VEC][W];
        double sc[PASS == 2 ? U : 1][2];  // column pass: lse and delta of the gathered rows
        double bias[BIAS ? 1 : 0];        // BIAS: bias[e + umine], the nonzero whose score this lane holds after the butterfly
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
    auto load_bias = [&](auto full, int e, Batch& b) {
        constexpr bool FULL = decltype(full)::value;
        if constexpr (BIAS) {
            const int mine = e + (lig / SUB) % U;
            b.bias[0] = (FULL || mine < end) ? a.bias[mine] : 0.0;
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
            for (int h = 0; h < 2; h++)
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
            if constexpr (PASS == 2) {
                b.sc[u][0] = 0.0;
                b.sc[u][1] = 0.0;
                if (live) load_w_global<2>(b.sc[u], rowp, 2u * half_bytes);  // (16-byte aligned: an even pitch, 2 fp even)
            }
        }
    };
    // this lane's part of <p, y> over its columns
    auto dot_part = [&](const double (&p)[VEC][W], const double (&y)[VEC][W]) {
        double s = 0.0;
#pragma unroll
        for (int v = 0; v < VEC; v++)
#pragma unroll
            for (int w = 0; w < W; w++) s = fma(p[v][w], y[v][w], s);
        return s;
    };
    auto compute = [&](auto full, int e, const Batch& b) {
        constexpr bool FULL = decltype(full)::value;
        double d[NR];
#pragma unroll
        for (int u = 0; u < U; u++) {
            d[u] = dot_part(x, b.y[u][0]);
            if constexpr (PASS != 0) d[U + u] = dot_part(z, b.y[u][1]);
        }
        const double r = group_multi_reduce<LPR, NR>(d, lig);  // reduction number lig / SUB
        const int umine = (lig / SUB) % U;
        const bool have = FULL || e + umine < end;
        if constexpr (PASS == 0) {
            // the online-softmax step of kFusedSoftmax (process_row), nonzero by nonzero in row order
            double sb = scale * r;
            if constexpr (BIAS) sb += b.bias[0];
            const double s = have ? sb : -__builtin_inf();
            if (a.values != nullptr && have && lig % SUB == 0) a.values[e + umine] = s;
            double run = m_run, mprev = m_run, mcur = m_run;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const double t = group_bcast<LPR>(s, u * SUB);
                const double nx = t > run ? t : run;
                if (umine == u) { mprev = run; mcur = nx; }
                run = nx;
            }
            const double fac = (mcur == mprev) ? 1.0 : (mprev == -__builtin_inf() ? 0.0 : exp(mprev - mcur));
            const double pw = have ? exp(s - mcur) : 0.0;
            m_run = run;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const double fu = group_bcast<LPR>(fac, u * SUB);
                const double pu = group_bcast<LPR>(pw, u * SUB);
                if (fu != 1.0) {  // the running max rose (uniform over the group)
#pragma unroll
                    for (int v = 0; v < VEC; v++)
#pragma unroll
                        for (int w = 0; w < W; w++) acc[v][w] *= fu;
                    l_run *= fu;
                }
                l_run += pu;
#pragma unroll
                for (int v = 0; v < VEC; v++)
#pragma unroll
                    for (int w = 0; w < W; w++) acc[v][w] = fma(pu, b.y[u][1][v][w], acc[v][w]);
            }
        } else {
            // the lower half of the group holds the <Q, K>'s, the upper half the <dZ, V>'s of the same nonzeros
            const double o = shfl_xor_f64(r, LPR / 2);
            const bool lower = lig < LPR / 2;
            const double qk = lower ? r : o, da = lower ? o : r;
            double l = lse_i, dl = delta_i;
            if constexpr (PASS == 2) {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (u == umine) {
                        l = b.sc[u][0];
                        dl = b.sc[u][1];
                    }
            }
            // BIAS: exp((scale qk - lse) + bias).  The parent's expression first, so that a zero bias leaves the plain pass's bits; the bias
            // behind it, so that an edge at -1e300 gives exp(-1e300) = 0 next to a moderate lse and exp(0) = 1 alone in its row, whose lse
            // the forward pass stored as -1e300 (never lse - bias: in that row it would be 0 and p the unbiased exp(scale qk)).
            double ex = scale * qk - l;
            if constexpr (BIAS) ex += b.bias[0];
            double wp = exp(ex);
            double wg = scale * (wp * (da - dl));
            if constexpr (DBIAS) {
                if (have && lower && lig % SUB == 0) {
                    double* const d = a.dbias + (e + umine);
                    double gb = wp * (da - dl);
                    // (load, add, store: the product is rounded before the sum and never contracted into it, so that accumulating onto a
                    // vector is that vector plus the overwriting call's result to the bit)
                    asm volatile("" : "+v"(gb));
                    *d = a.accumulate ? *d + gb : gb;
                }
            }
            if (!have) {
                wp = 0.0;
                wg = 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const double gu = group_bcast<LPR>(wg, u * SUB);
#pragma unroll
                for (int v = 0; v < VEC; v++)
#pragma unroll
                    for (int w = 0; w < W; w++) acc[v][w] = fma(gu, b.y[u][0][v][w], acc[v][w]);
                if constexpr (PASS == 2) {
                    const double pu = group_bcast<LPR>(wp, u * SUB);
#pragma unroll
                    for (int v = 0; v < VEC; v++)
#pragma unroll
                        for (int w = 0; w < W; w++) acc2[v][w] = fma(pu, b.y[u][1][v][w], acc2[v][w]);
                }
            }
        }
        // pin the accumulation here (as process_row does): sunk to the end of the trip it would keep both gather buffers alive
#pragma unroll
        for (int v = 0; v < VEC; v++)
#pragma unroll
            for (int w = 0; w < W; w++) {
                asm volatile("" : "+v"(acc[v][w]));
                if constexpr (PASS == 2) asm volatile("" : "+v"(acc2[v][w]));
            }
    };
    const BoolTag<true> kFull;
    const BoolTag<false> kMasked;

    int e = beg;
    Batch ba, bb;
    if (e + U <= end) {
        int c0[U], c1[U];
        load_idx(kFull, e, c0);
        load_bias(kFull, e, ba);
        gather(kFull, c0, ba);
        for (;;) {
            const bool more = e + 2 * U <= end;
            if (more) {  // the next batch's gathers fly while this one is computed
                load_idx(kFull, e + U, c1);
                load_bias(kFull, e + U, bb);
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
                load_bias(kFull, e + U, ba);
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
        load_bias(kMasked, e, ba);
        gather(kMasked, c0, ba);
        compute(kMasked, e, ba);
    }

    if constexpr (PASS == 0) {
        // the row's state leaves with every launch, as in process_row
        if (lig == 0) {
            a.row_max[row] = m_run;
            a.row_sum[row] = l_run;
        }
        if (flags & kInternalEpilogue) {  // finish: o = acc / l through the activation into the head's column block, and lse; Out is scratch
            const bool live = l_run > 0.0;
            if (flags & HNH_ATTN_ADDEND) {  // act(o + addend), the addend read from the destination by the lane that overwrites it (wave-uniform)
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    double o[W];
#pragma unroll
                    for (int w = 0; w < W; w++) o[w] = 0.0;
                    if (act[v]) load_w_stream<W>(o, a.relu_dst + row * a.relu_ld + coff[v]);
#pragma unroll
                    for (int w = 0; w < W; w++) o[w] = attn_out_addend(live ? acc[v][w] / l_run : 0.0, o[w], flags);
                    if (act[v]) store_w_stream<W>(a.relu_dst + row * a.relu_ld + coff[v], o);
                }
            } else if (flags & kAttnActMask) {  // ELU / identity in the ReLU's place (wave-uniform)
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    double o[W];
#pragma unroll
                    for (int w = 0; w < W; w++) o[w] = live ? attn_out_act(acc[v][w] / l_run, flags) : 0.0;
                    if (act[v]) store_w_stream<W>(a.relu_dst + row * a.relu_ld + coff[v], o);
                }
            } else {
#pragma unroll
                for (int v = 0; v < VEC; v++) {
                    double o[W];
#pragma unroll
                    for (int w = 0; w < W; w++) o[w] = live ? fmax(acc[v][w] / l_run, 0.0) : 0.0;
                    if (act[v]) store_w_stream<W>(a.relu_dst + row * a.relu_ld + coff[v], o);
                }
            }
            if (lig == 0) a.lse[row] = live ? m_run + log(l_run) : 0.0;
            return;
        }
    }
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        if (!act[v]) continue;
        if (part_row != nullptr) {  // a hub row's segment [dK (0) | dV] (or dQ alone): added up in order afterwards
            store_w_stream<W>(part_row + coff[v], acc[v]);
            if constexpr (PASS == 2) store_w_stream<W>(part_row + a.fp + coff[v], acc2[v]);
        } else {
            store_w_stream<W>(a.Out + row * a.ld_out + coff[v], acc[v]);
            if constexpr (PASS == 2) store_w_stream<W>(a.Out2 + row * a.ld_out2 + coff[v], acc2[v]);
        }
    }
}

// the instance's name for the shells of hnh_attn_dispatch.hpp (attn_rows_kernel, attn_segments_kernel)
template <int PASS, int LPR, int VEC, int W, bool EXACT, bool BIAS = false, bool DBIAS = false>
struct AqPass {
    using Args = AqArgsOf<BIAS, DBIAS>;
    static constexpr int lpr = LPR;
    static __device__ __forceinline__ void run(int64_t row, int beg, int end, const int32_t* __restrict__ colidx, const Args& a, unsigned flags, int lig,
                                               double* part_row) {
        attn_qkv_process<PASS, LPR, VEC, W, EXACT, BIAS, DBIAS>(row, beg, end, colidx, a, flags, lig, part_row);
    }
};

// BIAS: the entry points of include/hnh_attn_edge.h, with `bias` in the block's numbering; DBIAS: those of include/hnh_attn_edge_grad.h, with
// `dbias` in the same numbering
template <int PASS, bool BIAS = false, bool DBIAS = false>
int attn_qkv_dispatch(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* g, unsigned flags, const hnh_csr_window* win, int stream,
                      const char* who, const double* bias = nullptr, double* dbias = nullptr, int accumulate = 0) {
    HNH_ENTER(ctx, stream);
    if (int rc = attn_dispatch_head(ctx, b, g != nullptr, g ? g->f : 0, HNH_ATTN_QKV_MAX_F, "HNH_ATTN_QKV_MAX_F", PASS == 0, flags, win, who)) return rc;
    // (behind the head: the parents' refusals, the width limit among them, come first and with their codes)
    if (BIAS && b->rowptr != nullptr && bias == nullptr) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null bias");
    if (DBIAS && b->rowptr != nullptr && dbias == nullptr) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null dbias");
    const bool finish = PASS == 0 && (flags & HNH_ATTN_FINISH) != 0;
    if (b->rows == 0) return HNH_OK;
    const int f = g->f, fp = f + (f & 1);
    if (!g->Out || g->ld_out < f) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad output");
    if (PASS == 2 && (!g->Out2 || g->ld_out2 < f || g->Out2 == g->Out)) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad second output");
    if (PASS == 0 && (!g->row_max || !g->row_sum || !g->lse || !g->relu_dst || g->relu_ld < f))
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad row state");
    AqArgsOf<BIAS, DBIAS> a;
    if constexpr (BIAS) a.bias = bias;
    if constexpr (DBIAS) {
        a.dbias = dbias;
        a.accumulate = accumulate != 0;
    }
    a.X = g->X; a.X2 = g->X2; a.dZ = g->dZ; a.delta = g->delta; a.Y = g->Y; a.lse = g->lse; a.Out = g->Out; a.Out2 = g->Out2;
    a.row_max = g->row_max; a.row_sum = g->row_sum; a.relu_dst = g->relu_dst; a.values = PASS == 0 ? g->values : nullptr;
    a.ld_x = g->ld_x; a.ld_x2 = g->ld_x2; a.ld_dz = g->ld_dz; a.ld_y = g->ld_y; a.ld_out = g->ld_out; a.ld_out2 = g->ld_out2; a.relu_ld = g->relu_ld;
    a.f = f; a.fp = fp; a.scale = g->scale;
    hipStream_t st = ctx->streams[stream];
    const unsigned kflags = (flags & (HNH_FUSED_OUT_OVERWRITE | kAttnActMask | HNH_ATTN_ADDEND)) | (finish ? kInternalEpilogue : 0u);
    // a segment's partial result: dQ alone or [dK (0) | dV]; none for the forward pass, which walks hub rows whole
    const int64_t pitch = PASS == 0 ? 0 : (PASS == 2 ? 2 * fp : f);
    AttnSums sums;
    if (PASS != 0) sums.add(0, g->Out, g->ld_out, f);
    if (PASS == 2) sums.add(fp, g->Out2, g->ld_out2, f);
    if (b->rowptr == nullptr) {
        const AttnRowState state = {g->lse, g->Out, g->row_max, g->row_sum, g->relu_dst, g->ld_out, g->relu_ld, f};
        return attn_dispatch_no_nonzeros(ctx, st, b, kflags, PASS == 0 ? &state : nullptr, sums, who);
    }
    if (!b->col_idx || !g->X || !g->Y) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null pointer");
    if (g->ld_x < f) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": ld_x is narrower than f");
    if ((const double*)g->Out == g->X || (const double*)g->Out == g->Y || (PASS == 2 && ((const double*)g->Out2 == g->X || (const double*)g->Out2 == g->Y)))
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": an output aliases an input");
    // the packed operand (hnh_attn_grad.h): an even pitch and a 16-byte aligned base, whatever f is
    const int gather_w = HNH_ATTN_GRAD_PACKED_WIDTH(f, PASS == 2 ? 1 : 0);
    if (g->ld_y < gather_w || g->ld_y % 2 != 0 || !aligned16(g->Y))
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": the packed operand needs an even pitch of at least " + std::to_string(gather_w) +
                                                   " and a 16-byte aligned base");
    bool w2 = f % 2 == 0 && aligned16(g->X) && g->ld_x % 2 == 0 && aligned16(g->Out) && g->ld_out % 2 == 0;
    if (PASS == 0) w2 = w2 && aligned16(g->relu_dst) && g->relu_ld % 2 == 0;
    if (PASS == 1) {
        if (!g->dZ || g->ld_dz < f || !g->lse || !g->delta) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad dZ, lse or delta");
        if ((const double*)g->Out == g->dZ) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": an output aliases an input");
        w2 = w2 && aligned16(g->dZ) && g->ld_dz % 2 == 0;
    }
    if (PASS == 2) {
        if (!g->X2 || g->ld_x2 < f) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad own rows of V");
        if ((const double*)g->Out == g->X2 || (const double*)g->Out2 == g->X2)
            return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": an output aliases an input");
        w2 = w2 && aligned16(g->X2) && g->ld_x2 % 2 == 0 && aligned16(g->Out2) && g->ld_out2 % 2 == 0;
    }

    auto launch = [&](const LongCtl& lc, const int32_t* beg_ptr, const int32_t* end_ptr, unsigned fl, bool run_long) {
        return attn_launch_shape(f, w2, [&](auto l, auto v, auto w, auto ex) {
            return attn_launch<AqPass<PASS, decltype(l)::value, decltype(v)::value, decltype(w)::value, decltype(ex)::value, BIAS, DBIAS>, PASS == 0, false>(
                ctx, st, lc, b->rows, b->rowptr, beg_ptr, end_ptr, b->col_idx, a, fl, run_long, pitch, sums);
        });
    };
    return attn_dispatch_tail(ctx, st, stream, b, win, f, w2, pitch, gather_w, kflags, who, launch);
}

}  // namespace

extern "C" {

int hnh_attn_qkv_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, unsigned flags, const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<0>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_fwd_csr_p");
}

int hnh_attn_qkv_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, unsigned flags, const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<1>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_row_csr_p");
}

int hnh_attn_qkv_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, unsigned flags, const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<2>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_col_csr_p");
}

// ---- the per-edge bias (include/hnh_attn_edge.h)
int hnh_attn_qkv_bias_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, unsigned flags,
                                const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<0, true>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_bias_fwd_csr_p", bias);
}

int hnh_attn_qkv_bias_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, unsigned flags,
                                const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<1, true>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_bias_row_csr_p", bias);
}

int hnh_attn_qkv_bias_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, unsigned flags,
                                const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<2, true>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_bias_col_csr_p", bias);
}

// ---- the per-edge bias's gradient (include/hnh_attn_edge_grad.h)
int hnh_attn_qkv_bias_grad_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, double* dbias, int accumulate,
                                     unsigned flags, const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<1, true, true>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_bias_grad_row_csr_p", bias, dbias, accumulate);
}

int hnh_attn_qkv_bias_grad_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_qkv* args, const double* bias, double* dbias, int accumulate,
                                     unsigned flags, const hnh_csr_window* window, int stream) {
    return attn_qkv_dispatch<2, true, true>(ctx, b, args, flags, window, stream, "hnh_attn_qkv_bias_grad_col_csr_p", bias, dbias, accumulate);
}

}  // extern "C"
