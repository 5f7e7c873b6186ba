// Top-k of inner products for a batch of query rows, the merge of such lists and a row gather (include/hnh_topk.h).  Included at the end
// of hnh_grad.hip.
//
// topk_rows_kernel<QREG, VEC>: a WAVE owns 32 query rows (two 16-row A fragments) and one item range (blockIdx.y = the split); the four waves
// of a workgroup own 128 consecutive queries and the same range.  Item tiles of 64 rows of Y are the B operand of v_mfma_f64_16x16x4_f64
// (fragment maps as in gram_rows_kernel: A lane l = A[i = l & 15][k = l >> 4], B lane l = B[k = l >> 4][j = l & 15], C register r of lane l
// = C[(l >> 4) + 4 r][l & 15]): 2 x 4 accumulators per wave, the K loop in tiles of 16.
//   Both operands have k contiguous in memory, and the order of the k's inside a K tile is free as long as both agree, so lane l loads the
//   FOUR consecutive doubles Q[row l & 15][k0 + 4 (l >> 4) ..] and Y[item l & 15][k0 + 4 (l >> 4) ..] and MFMA step s of the tile
//   multiplies k = k0 + 4 (l >> 4) + s: a fragment load reads 16 rows x one whole 128-byte line, and neither operand goes through LDS.
//   The four waves stay on the same item tile (one barrier per tile), so Y's lines come to the last three from the vector L1.  The next K
//   tile's fragments are fetched under the MFMAs.  QREG (R <= 128): the wave's Q fragments stay in registers for the whole range;
//   otherwise they are re-read per item tile (from L1 / L2).  VEC: 16-byte
//   loads (R % 4 == 0 and both bases aligned); otherwise 8-byte loads.  The k-th product of a score is the same in both.  The K order is fixed per R: a score's bits depend on its two rows and R only.
//   Selection.  Every query row has, in LDS, its THRESHOLD (its current k-th candidate in the total order, or "nothing yet") and the
//   number of candidates collected.  An item tile whose 2048 scores all fail their thresholds costs one compare each and one ballot.
//   Otherwise the score tile goes to LDS and the wave walks its rows, lane l on item l of the tile: the entries that beat the threshold
//   and are not excluded (a binary search in the query's sorted list, for those entries only) are appended to the row's candidate buffer
//   in the workspace (`cap` entries: 128 for k <= 64, else 256), their places taken from a ballot.  A buffer that would overflow is
//   first cut back to its first k by a bitonic sort in LDS, which raises the threshold.  The total order is strict, so the surviving
//   set does not depend on arrival order.  At the end of the range every row is sorted once more and its first k go to the output
//   (splits == 1) or to the split's list, which topk_merge_kernel merges.
//   A candidate buffer is written and read back by the same wave only, through different lanes: __threadfence() between the two.
// topk_merge_kernel: one wave per query and group of up to `fan` lists; the kept k and as many incoming lists as fit in 256 entries are
// sorted in LDS, round by round.  More than kTopkMergeFan lists are merged in two levels.
#pragma once
#include <cstdint>
#include <string>
#include "hnh_topk.h"

namespace {

constexpr int kTopkWaves = 4, kTopkMI = 2, kTopkNJ = 4, kTopkBK = 16;
constexpr int kTopkRowsPerWave = 16 * kTopkMI, kTopkRowsPerGroup = kTopkWaves * kTopkRowsPerWave, kTopkItemTile = 16 * kTopkNJ;
constexpr int kTopkMaxCap = 2 * HNH_TOPK_MAX_K;
constexpr int kTopkMergeFan = 32;  // lists that one wave merges
constexpr int kTopkRegTiles = 8;  // QREG: K tiles of a row kept in registers (R <= 128)
constexpr int64_t kTopkNoId = 0x7fffffffffffffffLL;  // the id of an empty entry while it is sorted: it ranks behind every real one

// entries of a row's candidate buffer: a power of two that holds the kept k plus the 64 candidates one item tile can bring
__host__ __device__ inline int topk_cap(int k) { return k <= 64 ? 128 : 256; }

__device__ inline bool topk_before(double s, int64_t id, double t, int64_t tid) { return s > t || (s == t && id < tid); }

// the wave's LDS writes so far are visible to all of its lanes
// (fences of the LDS address space only: they must not wait for the global loads that are in flight for the next tile)
__device__ inline void topk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// bitonic sort of `cap` (a power of two, <= 256) entries in LDS by one wave, best first in the total order
__device__ inline void topk_sort(double* ss, int64_t* si, int cap, int lane) {
    for (int size = 2; size <= cap; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            topk_wave_sync();
            for (int t = lane; t < cap / 2; t += 64) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const double a = ss[lo], b = ss[hi];
                const int64_t ai = si[lo], bi = si[hi];
                const bool swap = (lo & size) == 0 ? topk_before(b, bi, a, ai) : topk_before(a, ai, b, bi);
                if (swap) {
                    ss[lo] = b; si[lo] = bi;
                    ss[hi] = a; si[hi] = ai;
                }
            }
        }
    topk_wave_sync();
}

template <bool QREG, bool VEC>
__global__ __launch_bounds__(64 * kTopkWaves) void topk_rows_kernel(const double* __restrict__ Q, int64_t nq, const double* __restrict__ Y, int64_t n,
                                                                     int R, int64_t id_base, const int64_t* __restrict__ excl_ptr,
                                                                     const int32_t* __restrict__ excl_idx, int k, int cap, int64_t split_len,
                                                                     double* cand_s, int64_t* cand_id, double* __restrict__ out_s,
                                                                     int64_t* __restrict__ out_id) {
    constexpr int MI = kTopkMI, NJ = kTopkNJ;
    __shared__ double sort_s[kTopkWaves][kTopkMaxCap];
    __shared__ int64_t sort_i[kTopkWaves][kTopkMaxCap];
    __shared__ double tile[kTopkWaves][kTopkRowsPerWave][kTopkItemTile];
    __shared__ double thr_s[kTopkWaves][kTopkRowsPerWave];
    __shared__ int64_t thr_i[kTopkWaves][kTopkRowsPerWave];
    __shared__ int cnt[kTopkWaves][kTopkRowsPerWave];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fk = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * kTopkWaves + wave) * kTopkRowsPerWave;  // the wave's first query
    const int64_t split = blockIdx.y;
    const int64_t j_begin = split * split_len < n ? split * split_len : n;
    const int64_t j_end = j_begin + split_len < n ? j_begin + split_len : n;
    const int ktiles = (R + kTopkBK - 1) / kTopkBK;
    double* ss = sort_s[wave];
    int64_t* si = sort_i[wave];

    // Four consecutive doubles of a row of X (Q or Y) from column kk on, zero where the row or the column does not exist.  Every load
    // is UNCONDITIONAL, from a clamped address (row 0, column 0 where the lane has no element), and a select drops what it brought: a load
    // inside a branch is waited for inside it, and the fetch for the next tile could not stay in flight under the MFMAs.
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

    // the selection state of the wave's 32 rows, in LDS: the threshold (the row's current k-th candidate, or "nothing yet") and the
    // number of candidates collected
    if (lane < kTopkRowsPerWave) {
        thr_s[wave][lane] = -__builtin_inf();
        thr_i[wave][lane] = kTopkNoId;
        cnt[wave][lane] = 0;
    }
    topk_wave_sync();
    const int64_t slot0 = split * nq;  // the candidate buffer of (split, row) is entry slot0 + row

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

        // ---- selection: register r of accumulator (i, j) is query row0 + 16 i + fk + 4 r, item jt + 16 j + fr
        bool any = false;
#pragma unroll
        for (int i = 0; i < MI; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int lrow = 16 * i + fk + 4 * r;
                const double ts = thr_s[wave][lrow];
                const int64_t ti = thr_i[wave][lrow];
                const bool row_ok = row0 + lrow < nq;
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    const int64_t col = jt + 16 * j + fr;
                    any |= row_ok && col < j_end && topk_before(acc[i][j][r], col, ts, ti);
                }
            }
        if (__any(any)) {
            // the score tile goes to LDS and the rows are walked one by one, lane l on item jt + l
#pragma unroll
            for (int i = 0; i < MI; i++)
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int j = 0; j < NJ; j++) tile[wave][16 * i + fk + 4 * r][16 * j + fr] = acc[i][j][r];
            topk_wave_sync();
            const int64_t col = jt + lane;
#pragma unroll 1
            for (int lrow = 0; lrow < kTopkRowsPerWave; lrow++) {
                const int64_t row = row0 + lrow;
                if (row >= nq) break;  // (uniform)
                const double s = tile[wave][lrow][lane];
                bool ok = col < j_end && topk_before(s, col, thr_s[wave][lrow], thr_i[wave][lrow]);
                if (!__any(ok)) continue;
                if (ok && excl_ptr != nullptr) {  // is col in the query's sorted list?
                    const int64_t e1 = excl_ptr[row + 1];
                    int64_t lo = excl_ptr[row], hi = e1;
                    while (lo < hi) {
                        const int64_t mid = lo + ((hi - lo) >> 1);
                        if ((int64_t)excl_idx[mid] < col) lo = mid + 1;
                        else hi = mid;
                    }
                    ok = !(lo < e1 && (int64_t)excl_idx[lo] == col);
                }
                const unsigned long long mask = __ballot(ok);
                if (mask == 0ull) continue;
                const int add = __popcll(mask);
                int have = cnt[wave][lrow];
                double* bs = cand_s + (slot0 + row) * cap;
                int64_t* bi = cand_id + (slot0 + row) * cap;
                if (have + add > cap) {
                    // the buffer would overflow: it is cut back to its first k, which raises the threshold (have > cap - 64 >= k)
                    __threadfence();  // the candidates were appended by other lanes of this wave
                    for (int e = lane; e < cap; e += 64) {
                        ss[e] = e < have ? bs[e] : -__builtin_inf();
                        si[e] = e < have ? bi[e] : kTopkNoId;
                    }
                    topk_sort(ss, si, cap, lane);
                    for (int e = lane; e < k; e += 64) {
                        bs[e] = ss[e];
                        bi[e] = si[e];
                    }
                    if (lane == 0) {
                        thr_s[wave][lrow] = ss[k - 1];
                        thr_i[wave][lrow] = si[k - 1];
                    }
                    have = k;
                }
                if (ok) {
                    const int pos = have + __popcll(mask & ((1ull << lane) - 1ull));
                    bs[pos] = s;
                    bi[pos] = col;
                }
                topk_wave_sync();  // every lane has read the row's count (and the scratch is free again)
                if (lane == 0) cnt[wave][lrow] = have + add;
            }
            topk_wave_sync();
        }
        __syncthreads();  // the workgroup's waves walk the item tiles together: Y's lines are fetched into the L1 once
    }

    // ---- the end of the range: every row's candidates sorted, the first k written out (ids made global, the empty tail -inf, -1)
    topk_wave_sync();
#pragma unroll 1
    for (int lrow = 0; lrow < kTopkRowsPerWave; lrow++) {
        const int64_t row = row0 + lrow;
        if (row >= nq) break;  // (uniform)
        const int have = cnt[wave][lrow];
        __threadfence();
        for (int e = lane; e < cap; e += 64) {
            ss[e] = e < have ? cand_s[(slot0 + row) * cap + e] : -__builtin_inf();
            si[e] = e < have ? cand_id[(slot0 + row) * cap + e] : kTopkNoId;
        }
        topk_sort(ss, si, cap, lane);
        for (int e = lane; e < k; e += 64) {
            const bool empty = si[e] == kTopkNoId;
            out_s[(slot0 + row) * k + e] = empty ? -__builtin_inf() : ss[e];
            out_id[(slot0 + row) * k + e] = empty ? (int64_t)-1 : id_base + si[e];
        }
        topk_wave_sync();
    }
}

// blockIdx.y = the group: lists [fan blockIdx.y, min(parts, fan (blockIdx.y + 1))) are merged into list blockIdx.y of the output
__global__ __launch_bounds__(64) void topk_merge_kernel(const double* __restrict__ in_s, const int64_t* __restrict__ in_id, int parts, int fan, int64_t nq,
                                                        int k, double* __restrict__ out_s, int64_t* __restrict__ out_id) {
    constexpr int cap = kTopkMaxCap;
    __shared__ double ss[kTopkMaxCap];
    __shared__ int64_t si[kTopkMaxCap];
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int first = fan * (int)blockIdx.y;
    in_s += (int64_t)first * nq * k;
    in_id += (int64_t)first * nq * k;
    out_s += (int64_t)blockIdx.y * nq * k;
    out_id += (int64_t)blockIdx.y * nq * k;
    parts = parts - first < fan ? parts - first : fan;
    const int per_round = (cap - k) / k;  // (>= 1: cap >= 2 k)
    for (int e = lane; e < k; e += 64) {
        ss[e] = -__builtin_inf();
        si[e] = kTopkNoId;
    }
    for (int p0 = 0; p0 < parts; p0 += per_round) {
        const int np = parts - p0 < per_round ? parts - p0 : per_round;
        for (int e = k + lane; e < cap; e += 64) {  // [0, k): the kept entries; [k, k + np k): the round's lists; the rest empty
            const int x = e - k, part = x / k;
            double s = -__builtin_inf();
            int64_t id = kTopkNoId;
            if (part < np) {
                const int64_t at = ((int64_t)(p0 + part) * nq + q) * k + (x - part * k);
                const int64_t got = in_id[at];
                if (got >= 0) {
                    id = got;
                    s = in_s[at];
                }
            }
            ss[e] = s;
            si[e] = id;
        }
        topk_sort(ss, si, cap, lane);
    }
    for (int e = lane; e < k; e += 64) {
        const bool empty = si[e] == kTopkNoId;
        out_s[q * k + e] = empty ? -__builtin_inf() : ss[e];
        out_id[q * k + e] = empty ? (int64_t)-1 : si[e];
    }
}

__global__ void take_rows_kernel(const double* __restrict__ X, int64_t rows, int R, const int64_t* __restrict__ idx, int64_t total, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int64_t q = e / R, src = idx[q];
    out[e] = (src >= 0 && src < rows) ? X[src * R + (e - q * R)] : 0.0;
}

// the number of item ranges when the caller leaves it to the library: enough workgroups for one per compute unit, ranges of at least
// 2048 items.  A function of the shapes only; the result does not depend on it.
inline int topk_auto_splits(int64_t nq, int64_t n) {
    const int64_t groups = (nq + kTopkRowsPerGroup - 1) / kTopkRowsPerGroup;
    int64_t s = groups > 0 ? 256 / groups : 1;
    if (s > n / 2048) s = n / 2048;
    if (s > HNH_TOPK_MAX_SPLITS) s = HNH_TOPK_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

// bytes of workspace with `splits` ranges: the candidate buffers, and the splits' lists when there are several
inline int64_t topk_work_bytes(int64_t nq, int k, int splits) {
    const int64_t slots = nq * splits;
    const int64_t mid = splits > kTopkMergeFan ? (splits + kTopkMergeFan - 1) / kTopkMergeFan : 0;  // the first level's lists
    return slots * topk_cap(k) * 16 + (splits > 1 ? slots * k * 16 : 0) + mid * nq * k * 16;
}

inline const char* topk_bad_shape(int64_t nq, int64_t n, int R, int k) {
    if (k < 1 || k > HNH_TOPK_MAX_K) return "k must be between 1 and HNH_TOPK_MAX_K = 128";
    if (R < 1 || R > HNH_TOPK_MAX_R) return "R must be between 1 and HNH_TOPK_MAX_R = 512";
    if (nq < 0 || n < 0) return "negative nq or n";
    if ((nq + kTopkRowsPerGroup - 1) / kTopkRowsPerGroup > 0x7fffffffLL) return "too many queries for one launch";
    return nullptr;
}

// `mid_s`, `mid_id`: room for ceil(parts / kTopkMergeFan) lists when parts > kTopkMergeFan, or null: one level whatever `parts`
int launch_topk_merge(hnh_ctx* ctx, hipStream_t st, const double* in_s, const int64_t* in_id, int parts, int64_t nq, int k, double* out_s, int64_t* out_id,
                      double* mid_s, int64_t* mid_id) {
    if (parts > kTopkMergeFan && mid_s != nullptr) {
        const int groups = (parts + kTopkMergeFan - 1) / kTopkMergeFan;
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)nq, (unsigned)groups), dim3(64), 0, st, in_s, in_id, parts, kTopkMergeFan, nq, k, mid_s, mid_id);
        in_s = mid_s;
        in_id = mid_id;
        parts = groups;
    }
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)nq, 1u), dim3(64), 0, st, in_s, in_id, parts, parts, nq, k, out_s, out_id);
    return hnh::check_hip(ctx, hipGetLastError(), "topk_merge_kernel launch");
}

}  // namespace

extern "C" {

int64_t hnh_topk_rows_f64_workspace(int64_t nq, int64_t n, int R, int k) {
    if (topk_bad_shape(nq, n, R, k) != nullptr) return -1;
    const int splits = topk_auto_splits(nq, n);
    return topk_work_bytes(nq, k, splits > 8 ? splits : 8);
}

int hnh_topk_rows_f64(hnh_ctx* ctx, const double* Q, int64_t nq, const double* Y, int64_t n, int R, int64_t id_base, const int64_t* excl_ptr,
                      const int32_t* excl_idx, int k, int splits, double* out_scores, int64_t* out_ids, void* work, int64_t work_bytes, int stream) {
    HNH_ENTER(ctx, stream);
    if (const char* bad = topk_bad_shape(nq, n, R, k)) return hnh::fail(ctx, HNH_ERR_INVALID, std::string("hnh_topk_rows_f64: ") + bad);
    if (splits < 0 || splits > HNH_TOPK_MAX_SPLITS)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_rows_f64: splits must be between 0 and HNH_TOPK_MAX_SPLITS = " + std::to_string(HNH_TOPK_MAX_SPLITS));
    // -1 marks an empty entry and the merge takes every negative id for one: the ids id_base .. id_base + n - 1 must be real ones
    if (id_base < 0 || id_base > INT64_MAX - n)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_rows_f64: id_base must be between 0 and INT64_MAX - n, not " + std::to_string(id_base));
    if (nq == 0) return HNH_OK;
    if (!Q || (n > 0 && !Y) || !out_scores || !out_ids || !work || (excl_ptr != nullptr && excl_idx == nullptr))
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_rows_f64: null pointer");
    if (splits == 0) splits = topk_auto_splits(nq, n);
    const int64_t need = topk_work_bytes(nq, k, splits);
    if (work_bytes < need)
        return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_rows_f64: the workspace is too small: " + std::to_string(work_bytes) + " bytes, " +
                                                   std::to_string(need) + " needed with " + std::to_string(splits) + " splits");
    if (!aligned16(work)) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_rows_f64: the workspace must be 16-byte aligned");
    hipStream_t st = ctx->streams[stream];
    const int cap = topk_cap(k);
    const int64_t slots = nq * splits, split_len = (n + splits - 1) / splits;
    double* cand_s = static_cast<double*>(work);
    int64_t* cand_id = reinterpret_cast<int64_t*>(cand_s + slots * cap);
    double* part_s = splits > 1 ? reinterpret_cast<double*>(cand_id + slots * cap) : out_scores;
    int64_t* part_id = splits > 1 ? reinterpret_cast<int64_t*>(part_s + slots * k) : out_ids;
    const bool vec = R % 4 == 0 && aligned16(Q) && aligned16(Y);  // 16-byte loads only where base and pitch allow
    const bool qreg = R <= kTopkBK * kTopkRegTiles;
    const dim3 grid((unsigned)((nq + kTopkRowsPerGroup - 1) / kTopkRowsPerGroup), (unsigned)splits);
#define HNH_TOPK_LAUNCH(QREG, VEC)                                                                                                                    \
    hipLaunchKernelGGL((topk_rows_kernel<QREG, VEC>), grid, dim3(64 * kTopkWaves), 0, st, Q, nq, Y, n, R, id_base, excl_ptr, excl_idx, k, cap, split_len, \
                       cand_s, cand_id, part_s, part_id)
    if (qreg && vec) HNH_TOPK_LAUNCH(true, true);
    else if (qreg) HNH_TOPK_LAUNCH(true, false);
    else if (vec) HNH_TOPK_LAUNCH(false, true);
    else HNH_TOPK_LAUNCH(false, false);
#undef HNH_TOPK_LAUNCH
    const int rc = hnh::check_hip(ctx, hipGetLastError(), "topk_rows_kernel launch");
    if (rc != HNH_OK || splits == 1) return rc;
    double* mid_s = part_s + 2 * slots * k;
    return launch_topk_merge(ctx, st, part_s, part_id, splits, nq, k, out_scores, out_ids, mid_s,
                             reinterpret_cast<int64_t*>(mid_s + (int64_t)((splits + kTopkMergeFan - 1) / kTopkMergeFan) * nq * k));
}

int hnh_topk_merge_f64(hnh_ctx* ctx, const double* in_scores, const int64_t* in_ids, int parts, int64_t nq, int k, double* out_scores, int64_t* out_ids,
                       int stream) {
    HNH_ENTER(ctx, stream);
    if (k < 1 || k > HNH_TOPK_MAX_K) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_merge_f64: k must be between 1 and HNH_TOPK_MAX_K = 128");
    if (parts < 1 || nq < 0 || nq > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_merge_f64: parts < 1, negative nq or too many queries");
    if (nq == 0) return HNH_OK;
    if (!in_scores || !in_ids || !out_scores || !out_ids) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_topk_merge_f64: null pointer");
    return launch_topk_merge(ctx, ctx->streams[stream], in_scores, in_ids, parts, nq, k, out_scores, out_ids, nullptr, nullptr);
}

int hnh_take_rows_f64(hnh_ctx* ctx, const double* X, int64_t rows, int R, const int64_t* idx, int64_t nq, double* out, int stream) {
    HNH_ENTER(ctx, stream);
    if (rows < 0 || nq < 0 || R < 1) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_take_rows_f64: negative rows or nq, or R < 1");
    if (nq == 0) return HNH_OK;
    if ((rows > 0 && !X) || !idx || !out) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_take_rows_f64: null pointer");
    const int64_t total = nq * R, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_INVALID, "hnh_take_rows_f64: too many elements for one launch");
    hipLaunchKernelGGL(take_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->streams[stream], X, rows, R, idx, total, out);
    return hnh::check_hip(ctx, hipGetLastError(), "take_rows_kernel launch");
}

}  // extern "C"
