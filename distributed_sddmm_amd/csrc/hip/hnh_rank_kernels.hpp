// Exact item ranks (include/hnh_rank.h): how many items rank before a target in the total order of include/hnh_topk.h, the scores of
// single pairs, and the subtraction of excluded entries.  Included at the end of hnh_grad.hip, after hnh_topk_kernels.hpp, whose
// constants, topk_before() and topk_wave_sync() it uses; nothing of that file is changed.
//
// rank_rows_kernel<QREG, VEC>: the COUNTING sibling of topk_rows_kernel.  The wave layout and the product loop are REPEATED from it and
// must stay in step with it: a wave owns 32 query rows (two 16-row A fragments) and one item range (blockIdx.y = the split), item tiles of
// 64 rows of Y are the B operand of v_mfma_f64_16x16x4_f64, 2 x 4 accumulators per wave, the K loop in tiles of 16, lane l loads the four
// consecutive doubles X[row l & 15][k0 + 4 (l >> 4) ..] of both operands and MFMA step s of the tile multiplies k = k0 + 4 (l >> 4) + s, the
// next fragments fetched under the MFMAs, QREG (R <= 128) keeps the wave's Q fragments in registers, VEC uses 16-byte loads.  So an
// accumulator holds the very bits that topk_rows_kernel selects by and returns.
//   Counting.  Every query row has up to HNH_RANK_MAX_TARGETS = 16 thresholds in LDS: the target's score and `rel` = its id - id_base (the
//   item row of Y that would carry the target's id; 0 where the id lies below the range: no row is before row 0), unused places
//   (+infinity, 0), which nothing ranks before.  Register r of accumulator (i, j) of lane l is query row 16 i + (l >> 4) + 4 r and item
//   jt + 16 j + (l & 15): the 16 lanes that share l >> 4 hold 16 items of ONE query row.  For target t the lanes compare their four items
//   of the row with the row's threshold t; the ballot of a compare holds the answers of four query rows, sixteen bits each, and the lane
//   with (l & 15) == t adds the popcount of its row's sixteen bits to ITS counter of that row: lane (l >> 4, t) owns the counts of target t
//   of the eight rows 16 i + (l >> 4) + 4 r, in registers.  The loop over t ends at the largest number of targets of the wave's rows.  No
//   score tile goes to LDS or memory, nothing is searched, and nothing is written before the end of the range, when every owner writes
//   its counts to `counts` (splits == 1) or to the split's slab of the workspace, which rank_sum_kernel adds up in split order.
// pair_scores_kernel<VEC>: a wave takes 16 pairs: pair p's query row is row p of the A fragment and its item row column p of the B
//   fragment, with the same loads and the same MFMA steps, and the diagonal of C is read.  Fifteen sixteenths of the products are thrown
//   away; the pairs are few.
// rank_exclude_kernel: one wave per query walks the query's excluded entries for each of its targets.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "hnh_rank.h"

namespace {

constexpr int kRankT = HNH_RANK_MAX_TARGETS;
static_assert(kRankT == 16, "lane (l & 15) == t owns target t of its rows");
static_assert(HNH_RANK_MAX_R == HNH_TOPK_MAX_R, "one product loop, one widest row");

template <bool QREG, bool VEC>
__global__ __launch_bounds__(64 * kTopkWaves) void rank_rows_kernel(const double* __restrict__ Q, int64_t nq, const double* __restrict__ Y, int64_t n, int R,
                                                                     int64_t id_base, const int64_t* __restrict__ tgt_ptr,
                                                                     const double* __restrict__ tgt_score, const int64_t* __restrict__ tgt_id,
                                                                     int64_t ntargets, int64_t split_len, int64_t* __restrict__ out) {
    constexpr int MI = kTopkMI, NJ = kTopkNJ;
    __shared__ double thr_s[kTopkWaves][kTopkRowsPerWave][kRankT];
    __shared__ int64_t thr_rel[kTopkWaves][kTopkRowsPerWave][kRankT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fk = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kTopkWaves + wave) * kTopkRowsPerWave;  // the wave's first query
    const int64_t split = blockIdx.y;
    const int64_t j_begin = split * split_len < n ? split * split_len : n;
    const int64_t j_end = j_begin + split_len < n ? j_begin + split_len : n;
    const int ktiles = (R + kTopkBK - 1) / kTopkBK;

    // ---- the product loop's loads: as in topk_rows_kernel (every load unconditional, from a clamped address, dropped by a select)
    auto load4 = [&](const double* X, int64_t row, bool row_ok, int kk, double* dst) {
        const double* base = X + (row_ok ? row : (int64_t)0) * R;
        if constexpr (VEC) {  // (R % 4 == 0: the four columns exist together)
            const bool ok = row_ok && kk < R;
            const int at = kk < R ? kk : 0;
            const double2 lo = *reinterpret_cast<const double2*>(base + at);
            const double2 hi = *reinterpret_cast<const double2*>(base + at + 2);
            dst[0] = ok ? lo.x : 0.0; dst[1] = ok ? lo.y : 0.0; dst[2] = ok ? hi.x : 0.0; dst[3] = ok ? hi.y : 0.0;
        } else {
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) v[q] = base[kk + q < R ? kk + q : 0];
#pragma unroll
            for (int q = 0; q < 4; q++) dst[q] = (row_ok && kk + q < R) ? v[q] : 0.0;
        }
    };
    auto fetch_a = [&](int t, double (*dst)[4]) {
#pragma unroll
        for (int i = 0; i < MI; i++) load4(Q, row0 + 16 * i + fr, row0 + 16 * i + fr < nq, t * kTopkBK + 4 * fk, dst[i]);
    };
    auto fetch_b = [&](int64_t jt, int t, double (*dst)[4]) {
#pragma unroll
        for (int j = 0; j < NJ; j++) load4(Y, jt + 16 * j + fr, jt + 16 * j + fr < j_end, t * kTopkBK + 4 * fk, dst[j]);
    };

    double aq[QREG ? kTopkRegTiles : 1][MI][4];
    if constexpr (QREG) {
#pragma unroll
        for (int t = 0; t < kTopkRegTiles; t++)
            if (t < ktiles) fetch_a(t, aq[t]);
    }

    // ---- the thresholds of the wave's 32 rows, in LDS; `most` = the largest number of targets of one of them (uniform)
    int mine = 0;  // lanes 0 .. 31: the number of targets of row row0 + lane
    for (int e = lane; e < kTopkRowsPerWave * kRankT; e += 64) {
        const int lrow = e / kRankT, t = e - lrow * kRankT;
        const int64_t row = row0 + lrow;
        double s = __builtin_inf();
        int64_t rel = 0;
        if (row < nq) {
            const int64_t t0 = tgt_ptr[row], t1 = tgt_ptr[row + 1];
            if (t0 + t < t1) {
                const int64_t id = tgt_id[t0 + t];
                s = tgt_score[t0 + t];
                rel = id > id_base ? id - id_base : 0;
            }
        }
        thr_s[wave][lrow][t] = s;
        thr_rel[wave][lrow][t] = rel;
    }
    if (lane < kTopkRowsPerWave && row0 + lane < nq) mine = (int)(tgt_ptr[row0 + lane + 1] - tgt_ptr[row0 + lane]);
    int most = 0;
    for (int t = 0; t < kRankT; t++)
        if (__any(mine > t)) most = t + 1;
    topk_wave_sync();

    int64_t cnt[MI][4];  // lane (fk, fr) owns target fr of the rows 16 i + fk + 4 r
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) cnt[i][r] = 0;

    double rb[NJ][4], ra[MI][4];
    if (j_begin < j_end && row0 < nq) {
        fetch_b(j_begin, 0, rb);
        if constexpr (!QREG) fetch_a(0, ra);
    }
    const bool live = row0 < nq;  // (uniform) a wave without queries only keeps the barriers
    for (int64_t jt = j_begin; jt < j_end; jt += kTopkItemTile) {
        if (!live) {
            __syncthreads();
            continue;
        }
        d4_t acc[MI][NJ];
#pragma unroll
        for (int i = 0; i < MI; i++)
#pragma unroll
            for (int j = 0; j < NJ; j++) acc[i][j] = (d4_t){0.0, 0.0, 0.0, 0.0};

        auto k_tile = [&](int t, double (*a)[4]) {
            double b[NJ][4];
#pragma unroll
            for (int j = 0; j < NJ; j++)
#pragma unroll
                for (int q = 0; q < 4; q++) b[j][q] = rb[j][q];
            // the next fragments, in flight during the MFMAs below: the next K tile, or the first one of the next item tile
            if (t + 1 < ktiles) fetch_b(jt, t + 1, rb);
            else if (jt + kTopkItemTile < j_end) fetch_b(jt + kTopkItemTile, 0, rb);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int i = 0; i < MI; i++)
#pragma unroll
                    for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][s], b[j][s], acc[i][j], 0, 0, 0);
        };
        if constexpr (QREG) {
#pragma unroll
            for (int t = 0; t < kTopkRegTiles; t++)
                if (t < ktiles) k_tile(t, aq[t]);
        } else {
            for (int t = 0; t < ktiles; t++) {
                double a[MI][4];
#pragma unroll
                for (int i = 0; i < MI; i++)
#pragma unroll
                    for (int q = 0; q < 4; q++) a[i][q] = ra[i][q];
                fetch_a(t + 1 < ktiles ? t + 1 : 0, ra);
                k_tile(t, a);
            }
        }

        // ---- counting: register r of accumulator (i, j) is query row0 + 16 i + fk + 4 r, item jt + 16 j + fr
        int64_t col[NJ];
        bool col_ok[NJ];
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            col[j] = jt + 16 * j + fr;
            col_ok[j] = col[j] < j_end;
        }
        for (int t = 0; t < most; t++) {  // (uniform)
#pragma unroll
            for (int i = 0; i < MI; i++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int lrow = 16 * i + fk + 4 * r;
                    const double ts = thr_s[wave][lrow][t];
                    const int64_t rel = thr_rel[wave][lrow][t];
                    int before = 0;
#pragma unroll
                    for (int j = 0; j < NJ; j++) {
                        const double s = acc[i][j][r];
                        const unsigned long long mask = __ballot(col_ok[j] && (s > ts || (s == ts && col[j] < rel)));
                        before += __popcll((mask >> (16 * fk)) & 0xffffull);
                    }
                    cnt[i][r] += fr == t ? before : 0;
                }
        }
        __syncthreads();  // the workgroup's waves walk the item tiles together: Y's lines are fetched into the L1 once
    }

    // ---- the end of the range: every owner writes its counts (a row without a target t has no owner of t)
    if (!live) return;
    out += split * ntargets;
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = row0 + 16 * i + fk + 4 * r;
            if (row < nq) {
                const int64_t t0 = tgt_ptr[row], t1 = tgt_ptr[row + 1];
                if (t0 + fr < t1) out[t0 + fr] = cnt[i][r];
            }
        }
}

// counts[t] = the sum of the splits' slabs in split order (parts == 0: zero)
__global__ void rank_sum_kernel(const int64_t* __restrict__ slabs, int parts, int64_t ntargets, int64_t* __restrict__ counts) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntargets) return;
    int64_t sum = 0;
    for (int p = 0; p < parts; p++) sum += slabs[(int64_t)p * ntargets + t];
    counts[t] = sum;
}

template <bool VEC>
__global__ __launch_bounds__(64) void pair_scores_kernel(const double* __restrict__ Q, int64_t nq, const double* __restrict__ Y, int64_t n, int R,
                                                         const int64_t* __restrict__ pair_q, const int64_t* __restrict__ pair_j, int64_t npairs,
                                                         double* __restrict__ out) {
    const int lane = threadIdx.x, fr = lane & 15, fk = lane >> 4;
    const int64_t p = (int64_t)blockIdx.x * 16 + fr;  // the pair whose rows this lane loads
    const int ktiles = (R + kTopkBK - 1) / kTopkBK;
    int64_t q = -1, j = -1;
    if (p < npairs) {
        q = pair_q[p];
        j = pair_j[p];
    }
    const bool ok = q >= 0 && q < nq && j >= 0 && j < n;
    // as in topk_rows_kernel: four consecutive doubles of a row from column kk on, zero where the row or the column does not exist
    auto load4 = [&](const double* X, int64_t row, int kk, double* dst) {
        const double* base = X + (ok ? row : (int64_t)0) * R;
        if constexpr (VEC) {
            const bool has = ok && kk < R;
            const int at = kk < R ? kk : 0;
            const double2 lo = *reinterpret_cast<const double2*>(base + at);
            const double2 hi = *reinterpret_cast<const double2*>(base + at + 2);
            dst[0] = has ? lo.x : 0.0; dst[1] = has ? lo.y : 0.0; dst[2] = has ? hi.x : 0.0; dst[3] = has ? hi.y : 0.0;
        } else {
            double v[4];
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = base[kk + c < R ? kk + c : 0];
#pragma unroll
            for (int c = 0; c < 4; c++) dst[c] = (ok && kk + c < R) ? v[c] : 0.0;
        }
    };
    d4_t acc = (d4_t){0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < ktiles; t++) {
        double a[4], b[4];
        load4(Q, q, t * kTopkBK + 4 * fk, a);
        load4(Y, j, t * kTopkBK + 4 * fk, b);
#pragma unroll
        for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc, 0, 0, 0);
    }
    // C[p][p] is register p >> 2 of the lane with l & 15 == p and l >> 4 == p & 3
    const int r = fr >> 2;
    const double diag = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    if (p < npairs && fk == (fr & 3)) out[p] = ok ? diag : 0.0;
}

__global__ __launch_bounds__(64) void rank_exclude_kernel(const int64_t* __restrict__ excl_ptr, const double* __restrict__ excl_score,
                                                          const int64_t* __restrict__ excl_id, const int64_t* __restrict__ tgt_ptr,
                                                          const double* __restrict__ tgt_score, const int64_t* __restrict__ tgt_id,
                                                          int64_t* __restrict__ counts) {
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t e0 = excl_ptr[q], e1 = excl_ptr[q + 1];
    if (e0 >= e1) return;  // (uniform)
    for (int64_t t = tgt_ptr[q]; t < tgt_ptr[q + 1]; t++) {
        const double ts = tgt_score[t];
        const int64_t ti = tgt_id[t];
        long long before = 0;
        for (int64_t e = e0 + lane; e < e1; e += 64) before += topk_before(excl_score[e], excl_id[e], ts, ti) ? 1 : 0;
        for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off);
        if (lane == 0) counts[t] -= before;
    }
}

// the number of item ranges when the caller leaves it to the library: a function of the shapes only (topk_auto_splits's rule: one
// workgroup per compute unit, ranges of at least 2048 items); the counts do not depend on it
inline int rank_auto_splits(int64_t nq, int64_t n) {
    const int64_t groups = (nq + kTopkRowsPerGroup - 1) / kTopkRowsPerGroup;
    int64_t s = groups > 0 ? 256 / groups : 1;
    if (s > n / 2048) s = n / 2048;
    if (s > HNH_RANK_MAX_SPLITS) s = HNH_RANK_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

// the copy of tgt_ptr (rounded up to 16 bytes), then the splits' slabs when there are several
inline int64_t rank_ptr_bytes(int64_t nq) { return ((nq + 1) * 8 + 15) / 16 * 16; }
inline int64_t rank_work_bytes(int64_t nq, int64_t ntargets, int splits) {
    return rank_ptr_bytes(nq) + (splits > 1 ? ((int64_t)splits * ntargets * 8 + 15) / 16 * 16 : 0);
}

inline const char* rank_bad_shape(int64_t nq, int64_t n, int64_t ntargets, int splits) {
    if (nq < 0 || n < 0 || ntargets < 0) return "negative nq, n or number of targets";
    if (ntargets > nq * HNH_RANK_MAX_TARGETS) return "more targets than HNH_RANK_MAX_TARGETS = 16 per query row";
    if (splits < 0 || splits > HNH_RANK_MAX_SPLITS) return "splits must be between 0 and HNH_RANK_MAX_SPLITS = 1024";
    if ((nq + kTopkRowsPerGroup - 1) / kTopkRowsPerGroup > 0x7fffffffLL) return "too many queries for one launch";
    return nullptr;
}

}  // namespace

extern "C" {

int hnh_pair_scores_f64(hnh_ctx* ctx, const double* Q, int64_t nq, const double* Y, int64_t n, int R, const int64_t* pair_q, const int64_t* pair_j,
                        int64_t npairs, double* out, int stream) {
    HNH_ENTER(ctx, stream);
    if (R < 1 || R > HNH_RANK_MAX_R) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_pair_scores_f64: R must be between 1 and HNH_RANK_MAX_R = 512");
    if (nq < 0 || n < 0 || npairs < 0) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_pair_scores_f64: negative nq, n or npairs");
    if (npairs == 0) return HNH_OK;
    if ((nq > 0 && !Q) || (n > 0 && !Y) || !pair_q || !pair_j || !out) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_pair_scores_f64: null pointer");
    const int64_t blocks = (npairs + 15) / 16;
    if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_pair_scores_f64: too many pairs for one launch");
    hipStream_t st = ctx->streams[stream];
    if (nq == 0 || n == 0) {  // every pair is out of range: +0.0 is all bits zero
        hipLaunchKernelGGL(rank_sum_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, st, (const int64_t*)nullptr, 0, npairs,
                           reinterpret_cast<int64_t*>(out));
        return hnh::check_hip(ctx, hipGetLastError(), "rank_sum_kernel launch");
    }
    const bool vec = R % 4 == 0 && aligned16(Q) && aligned16(Y);
    if (vec) hipLaunchKernelGGL((pair_scores_kernel<true>), dim3((unsigned)blocks), dim3(64), 0, st, Q, nq, Y, n, R, pair_q, pair_j, npairs, out);
    else hipLaunchKernelGGL((pair_scores_kernel<false>), dim3((unsigned)blocks), dim3(64), 0, st, Q, nq, Y, n, R, pair_q, pair_j, npairs, out);
    return hnh::check_hip(ctx, hipGetLastError(), "pair_scores_kernel launch");
}

int64_t hnh_rank_rows_f64_workspace(int64_t nq, int64_t n, int64_t ntargets, int splits) {
    if (rank_bad_shape(nq, n, ntargets, splits) != nullptr) return -1;
    return rank_work_bytes(nq, ntargets, splits == 0 ? rank_auto_splits(nq, n) : splits);
}

int hnh_rank_rows_f64(hnh_ctx* ctx, const double* Q, int64_t nq, const double* Y, int64_t n, int R, int64_t id_base, const int64_t* tgt_ptr,
                      const double* tgt_score, const int64_t* tgt_id, int splits, int64_t* counts, void* work, int64_t work_bytes, int stream) {
    HNH_ENTER(ctx, stream);
    if (R < 1 || R > HNH_RANK_MAX_R) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: R must be between 1 and HNH_RANK_MAX_R = 512");
    if (nq > 0 && !tgt_ptr) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: null pointer");
    if (nq > 0 && tgt_ptr[0] != 0) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: tgt_ptr must start at 0");
    for (int64_t q = 0; q < nq; q++) {
        const int64_t have = tgt_ptr[q + 1] - tgt_ptr[q];
        if (have < 0) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: tgt_ptr must ascend");
        if (have > HNH_RANK_MAX_TARGETS)
            return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: query row " + std::to_string(q) + " has " + std::to_string(have) +
                                                       " targets, more than HNH_RANK_MAX_TARGETS = 16");
    }
    const int64_t ntargets = nq > 0 ? tgt_ptr[nq] : 0;
    if (const char* bad = rank_bad_shape(nq, n, ntargets, splits)) return hnh::fail(ctx, HNH_ERR_INVALID, std::string("hnh_rank_rows_f64: ") + bad);
    if (id_base < 0 || id_base > INT64_MAX - n)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: id_base must be between 0 and INT64_MAX - n, not " + std::to_string(id_base));
    if (nq == 0 || ntargets == 0) return HNH_OK;
    if (!Q || (n > 0 && !Y) || !tgt_score || !tgt_id || !counts || !work) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: null pointer");
    if (splits == 0) splits = rank_auto_splits(nq, n);
    const int64_t need = rank_work_bytes(nq, ntargets, splits);
    if (work_bytes < need)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: the workspace is too small: " + std::to_string(work_bytes) + " bytes, " +
                                                   std::to_string(need) + " needed with " + std::to_string(splits) + " splits");
    if (!aligned16(work)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_rows_f64: the workspace must be 16-byte aligned");
    hipStream_t st = ctx->streams[stream];
    const unsigned sum_blocks = (unsigned)((ntargets + 255) / 256);
    if (n == 0) {  // every count is 0
        hipLaunchKernelGGL(rank_sum_kernel, dim3(sum_blocks), dim3(256), 0, st, (const int64_t*)nullptr, 0, ntargets, counts);
        return hnh::check_hip(ctx, hipGetLastError(), "rank_sum_kernel launch");
    }
    int64_t* ptr_d = static_cast<int64_t*>(work);
    int64_t* slabs = reinterpret_cast<int64_t*>(static_cast<char*>(work) + rank_ptr_bytes(nq));
    HNH_TRY_HIP(ctx, hipMemcpyAsync(ptr_d, tgt_ptr, (size_t)(nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const int64_t split_len = (n + splits - 1) / splits;
    int64_t* dst = splits > 1 ? slabs : counts;
    const bool vec = R % 4 == 0 && aligned16(Q) && aligned16(Y);  // 16-byte loads only where base and pitch allow
    const bool qreg = R <= kTopkBK * kTopkRegTiles;
    const dim3 grid((unsigned)((nq + kTopkRowsPerGroup - 1) / kTopkRowsPerGroup), (unsigned)splits);
#define HNH_RANK_LAUNCH(QREG, VEC)                                                                                                              \
    hipLaunchKernelGGL((rank_rows_kernel<QREG, VEC>), grid, dim3(64 * kTopkWaves), 0, st, Q, nq, Y, n, R, id_base, (const int64_t*)ptr_d, tgt_score, \
                       tgt_id, ntargets, split_len, dst)
    if (qreg && vec) HNH_RANK_LAUNCH(true, true);
    else if (qreg) HNH_RANK_LAUNCH(true, false);
    else if (vec) HNH_RANK_LAUNCH(false, true);
    else HNH_RANK_LAUNCH(false, false);
#undef HNH_RANK_LAUNCH
    const int rc = hnh::check_hip(ctx, hipGetLastError(), "rank_rows_kernel launch");
    if (rc != HNH_OK || splits == 1) return rc;
    hipLaunchKernelGGL(rank_sum_kernel, dim3(sum_blocks), dim3(256), 0, st, (const int64_t*)slabs, splits, ntargets, counts);
    return hnh::check_hip(ctx, hipGetLastError(), "rank_sum_kernel launch");
}

int hnh_rank_exclude_f64(hnh_ctx* ctx, int64_t nq, const int64_t* excl_ptr, const double* excl_score, const int64_t* excl_id, const int64_t* tgt_ptr,
                         const double* tgt_score, const int64_t* tgt_id, int64_t* counts, int stream) {
    HNH_ENTER(ctx, stream);
    if (nq < 0 || nq > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_exclude_f64: negative nq or too many queries for one launch");
    if (nq == 0) return HNH_OK;
    if (!excl_ptr || !excl_score || !excl_id || !tgt_ptr || !tgt_score || !tgt_id || !counts)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_rank_exclude_f64: null pointer");
    hipLaunchKernelGGL(rank_exclude_kernel, dim3((unsigned)nq), dim3(64), 0, ctx->streams[stream], excl_ptr, excl_score, excl_id, tgt_ptr, tgt_score,
                       tgt_id, counts);
    return hnh::check_hip(ctx, hipGetLastError(), "rank_exclude_kernel launch");
}

}  // extern "C"
