// Additive (a1, a2) attention scores of the GAT (include/hnh_attn_additive.h): three sibling templates of the row kernel.  Included at the
// end of hnh_kernels.hip, after hnh_attn_grad_kernels.hpp, whose machinery they use as it is (AgUnroll; from hnh_attn_dispatch.hpp the row
// and segment kernels, the hub-row segment scheme and the dispatcher's head and tail) next to the row kernels' transposed butterfly and
// group broadcast; kept apart from process_row and attn_grad_process so that none of the existing instances changes by a register.
//
//   PASS 0  forward over S:        s_i and the row's softmax state in registers; gathers M_j = [A_j | s_j t_j]; z = s_i + t_j (no dot product,
//                                  no butterfly), the online-softmax step of kFusedSoftmax, acc = acc f + p A_j
//   PASS 1  backward row pass:     dZ_i, s_i, lse_i, delta_i in registers; gathers M_j; da = <dZ_i, A_j> (butterfly), gate, ds_i += dz
//   PASS 2  backward column pass:  A_j, t_j in registers; gathers Q_i = [dZ_i | s_i lse_i delta_i]; da = <A_j, dZ_i>, gate with the
//                                  gathered row's scalars, acc += a dZ_i, dt_j += dz
// Lane layout and batches as in attn_grad_process: U nonzeros per batch in one of two register buffers; lane group lig / SUB owns
// nonzero lig / SUB of the batch for the per-nonzero scalar work (one exp per lane and batch), whose results are handed round with group
// broadcasts.  The scalars of a gathered row come with one 16-byte load from column fp of that row.
#pragma once

namespace {

struct AaArgs {  // hnh_attn_add as the kernels take it
    const double* M;
    const double* dZ;
    const double* delta;
    const double* Y;
    double* lse;
    double* Out;
    double* vec;
    double* row_max;
    double* row_sum;
    double* relu_dst;
    int64_t ld_m, ld_dz, ld_y, ld_out, ld_vec, relu_ld;
    int f, fp;  // fp = f rounded up to even: column of the scalars in a scored / packed row
    double alpha;
};

// DROP instances (include/hnh_attn_dropout.h): the same arguments plus the mask's key.  A separate type, so that the plain instances'
// kernel arguments stay as they are.
struct AaDropArgs : AaArgs {
    unsigned key0, key1;  // seed, low and high word
    unsigned w2;          // layer * 65536 + head
    unsigned threshold;   // keep iff word 0 >= threshold
    double scale;         // 1 / (1 - p)
    int64_t row_id0;      // global id of the block's row 0
};
template <bool DROP> struct AaKernelArgs { using type = AaArgs; };
template <> struct AaKernelArgs<true> { using type = AaDropArgs; };

// Philox-4x32-10, word 0 (the contract of include/hnh_attn_dropout.h)
__device__ __forceinline__ unsigned philox_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// The column pass's DROP instances that would unroll by 8 take 4: at 8 the instances of f = 64 (255 VGPRs without the mask), f = 128 and
// the 8-byte-lane one of f <= 128 do not fit 256 VGPRs (the compiler moves 6 - 10 values to AGPRs and one wave per SIMD is left).
template <int PASS, int LPR, int VEC, int W, bool DROP>
struct AaUnroll {
    static constexpr int full = AgUnroll<0, LPR, VEC, W>::value;
    static constexpr int value = (DROP && PASS == 2 && full == 8) ? 4 : full;
};

template <int PASS, int LPR, int VEC, int W, bool EXACT, bool DROP = false>
__device__ __forceinline__ void attn_add_process(int64_t row, int beg, int end, const int32_t* __restrict__ colidx,
                                                 const typename AaKernelArgs<DROP>::type& a, unsigned flags, int lig, double* part_row) {
    constexpr int U = AaUnroll<PASS, LPR, VEC, W, DROP>::value;
    constexpr int SUB = LPR / U;  // lanes that own the same nonzero of a batch
    static_assert(SUB >= 1, "needs U <= LPR");
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

    double x[PASS == 0 ? 1 : VEC][W], acc[PASS == 1 ? 1 : VEC][W];
#pragma unroll
    for (int v = 0; v < VEC; v++) {
#pragma unroll
        for (int w = 0; w < W; w++) {
            if constexpr (PASS != 0) x[v][w] = 0.0;
            if constexpr (PASS != 1) acc[v][w] = 0.0;
        }
        if (act[v]) {
            if constexpr (PASS == 1) load_w_stream<W>(x[v], a.dZ + row * a.ld_dz + coff[v]);
            if constexpr (PASS == 2) load_w_stream<W>(x[v], a.M + row * a.ld_m + coff[v]);
            if constexpr (PASS != 1)
                if (!fresh) load_w_stream<W>(acc[v], a.Out + row * a.ld_out + coff[v]);
        }
    }
    // the own row's scalars: s_i (forward, row pass) or t_j (column pass); lse_i, delta_i (row pass)
    const double own = a.M[row * a.ld_m + a.fp + (PASS == 2 ? 1 : 0)];
    double lse_i = 0.0, delta_i = 0.0;
    if constexpr (PASS == 1) {
        lse_i = a.lse[row];
        delta_i = a.delta[row];
    }
    double m_run = -__builtin_inf(), l_run = 0.0;  // forward: the row's running max and sum (hnh_attention.h)
    double dsum = 0.0;                             // backward: the row's scalar sum (ds_i or dt_j)
    if constexpr (PASS == 0) {
        if (!fresh) {
            m_run = a.row_max[row];
            l_run = a.row_sum[row];
        }
    } else {
        if (!fresh) dsum = a.vec[row * a.ld_vec];
    }
    const uint64_t g_base = reinterpret_cast<uint64_t>(a.Y);
    const uint64_t ld_bytes = (uint64_t)a.ld_y * sizeof(double);
    const unsigned sc_bytes = (unsigned)a.fp * (unsigned)sizeof(double);

    struct Batch {
        double y[U][VEC][W];
        double sa[U][2];                    // [s t] of a scored row, [s lse] of a packed one
        double sb[(PASS == 2 || DROP) ? U : 1][2];  // [delta 0] of a packed row; DROP: [id 0] of a scored row, [delta id] of a packed one
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
            b.sa[u][0] = 0.0;
            b.sa[u][1] = 0.0;
            if (live) load_w_global<2>(b.sa[u], rowp, sc_bytes);  // (16-byte aligned: an even pitch, fp even)
            if constexpr (PASS == 2 || DROP) {
                b.sb[u][0] = 0.0;
                b.sb[u][1] = 0.0;
                if (live) load_w_global<2>(b.sb[u], rowp, sc_bytes + 16u);
            }
        }
    };
    auto compute = [&](auto full, int e, const Batch& b) {
        constexpr bool FULL = decltype(full)::value;
        const int umine = lig / SUB;
        const bool have = FULL || e + umine < end;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0;  // the scalars of this lane's nonzero
        [[maybe_unused]] double qid = 0.0;    // DROP: the gathered row's global id
#pragma unroll
        for (int u = 0; u < U; u++)
            if (u == umine) {
                q0 = b.sa[u][0];
                q1 = b.sa[u][1];
                if constexpr (PASS == 2) q2 = b.sb[u][0];
                if constexpr (DROP) qid = b.sb[u][PASS == 2 ? 1 : 0];
            }
        // DROP: c m_ij of this lane's nonzero, recomputed from (seed, layer, head, global row, global column): the same bits in the
        // forward pass, the row pass and (with the roles of own and gathered row exchanged) the column pass over S^T
        [[maybe_unused]] double keep = 1.0;
        if constexpr (DROP) {
            const unsigned own_id = (unsigned)(a.row_id0 + row), got_id = (unsigned)(unsigned long long)qid;
            const unsigned word = philox_word0(PASS == 2 ? got_id : own_id, PASS == 2 ? own_id : got_id, a.w2, 0u, a.key0, a.key1);
            keep = word >= a.threshold ? a.scale : 0.0;
        }
        const double z = PASS == 2 ? q0 + own : own + q1;  // s_i + t_j
        const double slope = z > 0.0 ? 1.0 : a.alpha;
        const double ev = z * slope;
        if constexpr (PASS == 0) {
            // the online-softmax step of kFusedSoftmax (process_row), nonzero by nonzero in row order
            const double s = have ? ev : -__builtin_inf();
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
            [[maybe_unused]] const double pwk = pw * keep;
            m_run = run;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const double fu = group_bcast<LPR>(fac, u * SUB);
                const double pu = group_bcast<LPR>(pw, u * SUB);
                double pa = pu;  // l takes every edge, acc the kept ones times c
                if constexpr (DROP) pa = group_bcast<LPR>(pwk, u * SUB);
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
                    for (int w = 0; w < W; w++) acc[v][w] = fma(pa, b.y[u][v][w], acc[v][w]);
            }
#pragma unroll
            for (int v = 0; v < VEC; v++)
#pragma unroll
                for (int w = 0; w < W; w++) asm volatile("" : "+v"(acc[v][w]));
        } else {
            double d[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                double sd = 0.0;
#pragma unroll
                for (int v = 0; v < VEC; v++)
#pragma unroll
                    for (int w = 0; w < W; w++) sd = fma(x[v][w], b.y[u][v][w], sd);
                d[u] = sd;
            }
            const double da = group_multi_reduce<LPR, U>(d, lig);  // reduction number lig / SUB
            const double l = PASS == 1 ? lse_i : q1, dl = PASS == 1 ? delta_i : q2;
            double wa = exp(ev - l);
            double wdz = wa * ((DROP ? keep * da : da) - dl) * slope;
            if constexpr (DROP) wa *= keep;  // (only dAgg reads it from here on)
            if (!have) {
                wa = 0.0;
                wdz = 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                dsum += group_bcast<LPR>(wdz, u * SUB);  // in row order
                if constexpr (PASS == 2) {
                    const double au = group_bcast<LPR>(wa, u * SUB);
#pragma unroll
                    for (int v = 0; v < VEC; v++)
#pragma unroll
                        for (int w = 0; w < W; w++) acc[v][w] = fma(au, b.y[u][v][w], acc[v][w]);
                }
            }
            if constexpr (PASS == 2) {
#pragma unroll
                for (int v = 0; v < VEC; v++)
#pragma unroll
                    for (int w = 0; w < W; w++) asm volatile("" : "+v"(acc[v][w]));
            }
            asm volatile("" : "+v"(dsum));
        }
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

    if constexpr (PASS == 0) {
        // the row's state leaves with every launch, as in process_row
        if (lig == 0) {
            a.row_max[row] = m_run;
            a.row_sum[row] = l_run;
        }
        if (flags & kInternalEpilogue) {  // finish: o = acc / l through the ReLU into the head's column block, and lse; Out is scratch
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
    if constexpr (PASS != 1) {
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            if (!act[v]) continue;
            if (part_row != nullptr) store_w_stream<W>(part_row + coff[v], acc[v]);  // a hub row's segment: added up in order afterwards
            else store_w_stream<W>(a.Out + row * a.ld_out + coff[v], acc[v]);
        }
    }
    if constexpr (PASS != 0) {
        if (lig == 0) {
            if (part_row != nullptr) part_row[PASS == 2 ? a.fp : 0] = dsum;
            else a.vec[row * a.ld_vec] = dsum;
        }
    }
}

// the instance's name for the shells of hnh_attn_dispatch.hpp (attn_rows_kernel, attn_segments_kernel)
template <int PASS, int LPR, int VEC, int W, bool EXACT, bool DROP = false>
struct AaPass {
    using Args = typename AaKernelArgs<DROP>::type;
    static constexpr int lpr = LPR;
    static __device__ __forceinline__ void run(int64_t row, int beg, int end, const int32_t* __restrict__ colidx, const Args& a, unsigned flags, int lig,
                                               double* part_row) {
        attn_add_process<PASS, LPR, VEC, W, EXACT, DROP>(row, beg, end, colidx, a, flags, lig, part_row);
    }
};

// a block without any nonzero, forward: the state reset of HNH_FUSED_OUT_OVERWRITE and the finish, as attn_add_process does them for a
// row whose piece is empty (one wave per row).  ACT: the finish applies ELU / the identity (flags) instead of the ReLU, or adds the addend
// that waits in the destination (HNH_ATTN_ADDEND, any activation), its own instance
template <bool ACT>
__global__ __launch_bounds__(kBlock) void attn_add_empty_rows_kernel(int64_t rows, AaArgs a, unsigned flags) {
    const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / 64;
    const int lane = threadIdx.x % 64;
    if (row >= rows) return;
    const bool fresh = (flags & HNH_FUSED_OUT_OVERWRITE) != 0, finish = (flags & kInternalEpilogue) != 0;
    const double m = fresh ? -__builtin_inf() : a.row_max[row];
    const double l = fresh ? 0.0 : a.row_sum[row];
    for (int c = lane; c < a.f; c += 64) {
        const double v = fresh ? 0.0 : a.Out[row * a.ld_out + c];
        if (finish) {
            double* d = a.relu_dst + row * a.relu_ld + c;
            if (ACT && (flags & HNH_ATTN_ADDEND)) *d = attn_out_addend(l > 0.0 ? v / l : 0.0, *d, flags);
            else *d = l > 0.0 ? (ACT ? attn_out_act(v / l, flags) : fmax(v / l, 0.0)) : 0.0;
        } else a.Out[row * a.ld_out + c] = v;
    }
    if (lane == 0) {
        a.row_max[row] = m;
        a.row_sum[row] = l;
        if (finish) a.lse[row] = l > 0.0 ? m + log(l) : 0.0;
    }
}

// (declared in hnh_attn_dispatch.hpp) the forward passes of every family share the kernel above: it reads the row state and nothing else
int attn_dispatch_no_nonzeros(hnh_ctx* ctx, hipStream_t st, const hnh_csr_block* b, unsigned kflags, const AttnRowState* state, const AttnSums& sums,
                              const char* who) {
    if (b->nnz > 0) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null rowptr");
    if (state != nullptr) {
        if (!kflags) return HNH_OK;
        AaArgs e = {};
        e.lse = state->lse; e.Out = state->Out; e.row_max = state->row_max; e.row_sum = state->row_sum; e.relu_dst = state->relu_dst;
        e.ld_out = state->ld_out; e.relu_ld = state->relu_ld; e.f = state->f;
        const dim3 grid((unsigned)((b->rows * 64 + kBlock - 1) / kBlock));
        if (kflags & (kAttnActMask | HNH_ATTN_ADDEND)) hipLaunchKernelGGL(attn_add_empty_rows_kernel<true>, grid, dim3(kBlock), 0, st, b->rows, e, kflags);
        else hipLaunchKernelGGL(attn_add_empty_rows_kernel<false>, grid, dim3(kBlock), 0, st, b->rows, e, kflags);
        return hnh::check_hip(ctx, hipGetLastError(), "attn_add_empty_rows_kernel launch");
    }
    if (!(kflags & HNH_FUSED_OUT_OVERWRITE)) return HNH_OK;
    for (int i = 0; i < sums.n; i++) {
        const AttnSums::Sum& s = sums.s[i];
        hipLaunchKernelGGL(attn_grad_zero_rows_kernel, dim3(ew_grid(b->rows * s.width)), dim3(kBlock), 0, st, s.dst, s.ld, b->rows, s.width);
        if (int rc = hnh::check_hip(ctx, hipGetLastError(), "attn_grad_zero_rows_kernel launch")) return rc;
    }
    return HNH_OK;
}

// M[r, :] = [A_r (0) | <A_r, a1> <A_r, a2>], one wave per row
__global__ __launch_bounds__(kBlock) void attn_add_scores_kernel(double* __restrict__ M, int64_t ld_m, const double* __restrict__ A, int64_t ld_a,
                                                                 const double* __restrict__ a1, const double* __restrict__ a2, int64_t rows, int f, int fp) {
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
    }
}

// Q[r, :] = [dZ_r (0) | s_r lse_r delta_r 0], the layout of include/hnh_attn_additive.h
__global__ __launch_bounds__(kBlock) void attn_add_pack_kernel(double* __restrict__ Q, int64_t ld_q, const double* __restrict__ dZ, int64_t ld_dz,
                                                               const double* __restrict__ M, int64_t ld_m, const double* __restrict__ lse,
                                                               const double* __restrict__ delta, int64_t rows, int f, int fp) {
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
        Q[r * ld_q + c] = v;
    }
}

__global__ __launch_bounds__(kBlock) void attn_add_update_kernel(double* __restrict__ dA, int64_t ld_da, int64_t col0, const double* __restrict__ dAgg,
                                                                 int64_t ld_g, const double* __restrict__ D, int64_t ld_d, const double* __restrict__ a1,
                                                                 const double* __restrict__ a2, int64_t rows, int f) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * f;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / f;
        const int c = (int)(i % f);
        dA[r * ld_da + col0 + c] = fma(D[r * ld_d + 1], a2[c], fma(D[r * ld_d], a1[c], dAgg[r * ld_g + c]));
    }
}

template <int PASS, bool DROP = false>
int attn_add_dispatch(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* g, unsigned flags, const hnh_csr_window* win, int stream,
                      const char* who, const hnh_attn_drop* drop = nullptr) {
    HNH_ENTER(ctx, stream);
    if (int rc = attn_dispatch_head(ctx, b, g && (!DROP || drop), g ? g->f : 0, HNH_ATTN_ADD_MAX_F, "HNH_ATTN_ADD_MAX_F", PASS == 0, flags, win, who)) return rc;
    const bool finish = PASS == 0 && (flags & HNH_ATTN_FINISH) != 0;
    if (b->rows == 0) return HNH_OK;
    const int f = g->f, fp = f + (f & 1);
    if (PASS != 1 && (!g->Out || g->ld_out < f)) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad output");
    if (PASS != 0 && (!g->vec || g->ld_vec < 1)) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad scalar output");
    if (PASS == 0 && (!g->row_max || !g->row_sum || !g->lse || !g->relu_dst || g->relu_ld < f))
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad row state");
    typename AaKernelArgs<DROP>::type a;
    if constexpr (DROP) {
        // ids travel as 32-bit counter words: the block's own rows and (the operand's ids are the caller's) nothing else is checked here
        if (drop->row_id0 < 0 || drop->row_id0 + b->rows > 0x100000000LL)
            return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": the block's global row ids do not fit 32 bits");
        a.key0 = (unsigned)(drop->seed & 0xffffffffu);
        a.key1 = (unsigned)(drop->seed >> 32);
        a.w2 = drop->w2;
        a.threshold = drop->threshold;
        a.scale = drop->scale;
        a.row_id0 = drop->row_id0;
    }
    a.M = g->M; a.dZ = g->dZ; a.delta = g->delta; a.Y = g->Y; a.lse = g->lse; a.Out = g->Out; a.vec = g->vec;
    a.row_max = g->row_max; a.row_sum = g->row_sum; a.relu_dst = g->relu_dst;
    a.ld_m = g->ld_m; a.ld_dz = g->ld_dz; a.ld_y = g->ld_y; a.ld_out = g->ld_out; a.ld_vec = g->ld_vec; a.relu_ld = g->relu_ld;
    a.f = f; a.fp = fp; a.alpha = g->leaky_alpha;
    hipStream_t st = ctx->streams[stream];
    const unsigned kflags = (flags & (HNH_FUSED_OUT_OVERWRITE | kAttnActMask | HNH_ATTN_ADDEND)) | (finish ? kInternalEpilogue : 0u);
    // a segment's partial result: [dAgg (0) | dt] (column pass) or ds alone; none for the forward pass, which walks hub rows whole
    const int64_t pitch = PASS == 0 ? 0 : (PASS == 2 ? fp + 2 : 2);
    AttnSums sums;
    if (PASS == 2) sums.add(0, g->Out, g->ld_out, f);
    if (PASS != 0) sums.add(PASS == 2 ? fp : 0, g->vec, g->ld_vec, 1);
    if (b->rowptr == nullptr) {
        const AttnRowState state = {g->lse, g->Out, g->row_max, g->row_sum, g->relu_dst, g->ld_out, g->relu_ld, f};
        return attn_dispatch_no_nonzeros(ctx, st, b, kflags, PASS == 0 ? &state : nullptr, sums, who);
    }
    if (!b->col_idx || !g->M || !g->Y) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null pointer");
    if (g->ld_m < fp + 2) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": ld_m is narrower than the scored width");
    // the gathered operand (hnh_attn_additive.h): an even pitch and a 16-byte aligned base, whatever f is
    const int gather_w = PASS == 2 ? HNH_ATTN_ADD_PACKED_WIDTH(f) : (DROP ? HNH_ATTN_DROP_SCORED_WIDTH(f) : HNH_ATTN_ADD_SCORED_WIDTH(f));
    if (g->ld_y < gather_w || g->ld_y % 2 != 0 || !aligned16(g->Y))
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": the gathered operand needs an even pitch of at least " + std::to_string(gather_w) +
                                                   " and a 16-byte aligned base");
    if (PASS != 1 && ((const double*)g->Out == g->M || (const double*)g->Out == g->Y))
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": Out aliases an input");
    bool w2 = f % 2 == 0;
    if (PASS == 0) w2 = w2 && aligned16(g->Out) && g->ld_out % 2 == 0 && aligned16(g->relu_dst) && g->relu_ld % 2 == 0;
    if (PASS == 1) {
        if (!g->dZ || g->ld_dz < f || !g->lse || !g->delta) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": bad dZ, lse or delta");
        w2 = w2 && aligned16(g->dZ) && g->ld_dz % 2 == 0;
    }
    if (PASS == 2) w2 = w2 && aligned16(g->M) && g->ld_m % 2 == 0 && aligned16(g->Out) && g->ld_out % 2 == 0;

    auto launch = [&](const LongCtl& lc, const int32_t* beg_ptr, const int32_t* end_ptr, unsigned fl, bool run_long) {
        return attn_launch_shape(f, w2, [&](auto l, auto v, auto w, auto ex) {
            return attn_launch<AaPass<PASS, decltype(l)::value, decltype(v)::value, decltype(w)::value, decltype(ex)::value, DROP>, PASS == 0, true>(
                ctx, st, lc, b->rows, b->rowptr, beg_ptr, end_ptr, b->col_idx, a, fl, run_long, pitch, sums);
        });
    };
    return attn_dispatch_tail(ctx, st, stream, b, win, f, w2, pitch, gather_w, kflags, who, launch);
}

}  // namespace

extern "C" {

int hnh_attn_add_fwd_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, unsigned flags, const hnh_csr_window* window,
                           int stream) {
    return attn_add_dispatch<0>(ctx, b, args, flags, window, stream, "hnh_attn_add_fwd_csr_p");
}

int hnh_attn_add_row_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, unsigned flags, const hnh_csr_window* window,
                           int stream) {
    return attn_add_dispatch<1>(ctx, b, args, flags, window, stream, "hnh_attn_add_row_csr_p");
}

int hnh_attn_add_col_csr_p(hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* args, unsigned flags, const hnh_csr_window* window,
                           int stream) {
    return attn_add_dispatch<2>(ctx, b, args, flags, window, stream, "hnh_attn_add_col_csr_p");
}

int hnh_attn_add_scores_f64(hnh_ctx* ctx, double* M, int64_t ld_m, const double* A, int64_t ld_a, const double* a1, const double* a2,
                            int64_t rows, int f, int stream) {
    HNH_ENTER(ctx, stream);
    if (int rc = check_common(ctx, rows, f, "hnh_attn_add_scores_f64")) return rc;
    const int fp = f + (f & 1);
    if (ld_m < fp + 2 || ld_m % 2 != 0 || ld_a < f) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_add_scores_f64: bad pitch");
    if (rows == 0) return HNH_OK;
    if (!M || !A || !a1 || !a2 || M == A) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_add_scores_f64: null or aliased pointer");
    hipLaunchKernelGGL(attn_add_scores_kernel, dim3((unsigned)((rows * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->streams[stream], M, ld_m, A, ld_a,
                       a1, a2, rows, f, fp);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_add_scores_kernel launch");
}

int hnh_attn_add_pack_f64(hnh_ctx* ctx, double* Q, int64_t ld_q, const double* dZ, int64_t ld_dz, const double* M, int64_t ld_m,
                          const double* lse, const double* delta, int64_t rows, int f, int stream) {
    HNH_ENTER(ctx, stream);
    if (int rc = check_common(ctx, rows, f, "hnh_attn_add_pack_f64")) return rc;
    const int fp = f + (f & 1);
    if (ld_q < fp + 4 || ld_q % 2 != 0 || ld_dz < f || ld_m < fp + 2) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_add_pack_f64: bad pitch");
    if (rows == 0) return HNH_OK;
    if (!Q || !dZ || !M || !lse || !delta) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_add_pack_f64: null pointer");
    hipLaunchKernelGGL(attn_add_pack_kernel, dim3(ew_grid(rows * (fp + 4))), dim3(kBlock), 0, ctx->streams[stream], Q, ld_q, dZ, ld_dz, M, ld_m, lse, delta,
                       rows, f, fp);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_add_pack_kernel launch");
}

int hnh_attn_add_update_f64(hnh_ctx* ctx, double* dA, int64_t ld_da, int64_t col0, const double* dAgg, int64_t ld_g, const double* D,
                            int64_t ld_d, const double* a1, const double* a2, int64_t rows, int f, int stream) {
    HNH_ENTER(ctx, stream);
    if (int rc = check_common(ctx, rows, f, "hnh_attn_add_update_f64")) return rc;
    if (col0 < 0 || ld_da < col0 + f || ld_g < f || ld_d < 2) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_add_update_f64: bad pitch");
    if (rows == 0) return HNH_OK;
    if (!dA || !dAgg || !D || !a1 || !a2) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_attn_add_update_f64: null pointer");
    hipLaunchKernelGGL(attn_add_update_kernel, dim3(ew_grid(rows * f)), dim3(kBlock), 0, ctx->streams[stream], dA, ld_da, col0, dAgg, ld_g, D, ld_d, a1, a2,
                       rows, f);
    return hnh::check_hip(ctx, hipGetLastError(), "attn_add_update_kernel launch");
}

}  // extern "C"
