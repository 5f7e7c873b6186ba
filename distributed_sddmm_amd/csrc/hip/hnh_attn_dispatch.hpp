// What the attention passes share (hnh_attn_grad_kernels.hpp, hnh_attn_additive_kernels.hpp with its DROP instances, hnh_attn_v2_kernels.hpp):
// the row kernel and the hub-row segment kernel round a family's per-row process function, the ordered sum of the segments' partial rows,
// the launcher of the three, and the head and the tail of a dispatcher.  Included by the first of them, inside hnh_kernels.hip, whose plans,
// hub-row work lists, LDS pad and Infinity-Cache panels it drives; every pass keeps its own process function (attn_grad_process,
// attn_add_process, attn_v2_process: apart, so that none of their instances changes by a register), its own argument checks and its own
// kernel arguments.  A family names an instance to the shells with a tag type
//     struct Tag { using Args = <kernel arguments>;  static constexpr int lpr = <lanes per row>;
//                  static __device__ void run(row, beg, end, colidx, const Args&, flags, lig, part_row); };
// which is what a `rocprofv3 --kernel-trace --stats` listing shows: attn_rows_kernel<AgPass<1, 64, 2, 2, true>, false> and so on.
#pragma once

namespace {

template <int N>
struct IntTag { static constexpr int value = N; };

// the instance that fits (f, alignment): exact widths 64 / 128 / 256, every other width bounds-checked (16-byte lanes when even);
// go(LPR, VEC, W, EXACT) receives the four constants as tag types
template <typename Go>
int attn_launch_shape(int f, bool w2, Go&& go) {
#define HNH_ATTN_SHAPE(L, V, WW, EX) return go(IntTag<L>(), IntTag<V>(), IntTag<WW>(), BoolTag<EX>())
    if (w2) {
        if (f == 64) HNH_ATTN_SHAPE(32, 1, 2, true);
        if (f == 128) HNH_ATTN_SHAPE(64, 1, 2, true);
        if (f == 256) HNH_ATTN_SHAPE(64, 2, 2, true);
        if (f < 128) HNH_ATTN_SHAPE(64, 1, 2, false);
        HNH_ATTN_SHAPE(64, 2, 2, false);
    }
    if (f <= 64) HNH_ATTN_SHAPE(64, 1, 1, false);
    if (f <= 128) HNH_ATTN_SHAPE(64, 2, 1, false);
    HNH_ATTN_SHAPE(64, 4, 1, false);
#undef HNH_ATTN_SHAPE
}

// The row kernel: a group of P::lpr lanes per sparse row.  WHOLE: this pass walks hub rows whole and visits every row (a forward pass: a
// row's scores are combined in row order, and the reset and the finish apply to empty pieces too).
template <typename P, bool WHOLE>
__global__ __launch_bounds__(kBlock) void attn_rows_kernel(int64_t rows, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ beg_ptr,
                                                           const int32_t* __restrict__ end_ptr, const int32_t* __restrict__ colidx, typename P::Args a,
                                                           unsigned flags) {
    constexpr int LPR = P::lpr;
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
    if constexpr (!WHOLE) {
        if (flags & kInternalSplitLong) {  // hub rows go to the segment kernel, whose sums are ADDED to the row (as in row_kernel)
            int full = rowptr[row + 1] - rowptr[row];
            if constexpr (LPR == 64) full = __builtin_amdgcn_readfirstlane(full);
            if (full > long_row_of(flags)) {
                if (flags & HNH_FUSED_OUT_OVERWRITE) end = beg;  // an overwritten row has to start from zero
                else return;
            }
        }
        if (beg == end && !(flags & HNH_FUSED_OUT_OVERWRITE)) return;  // nothing to add
    }
    P::run(row, beg, end, colidx, a, flags, lig, nullptr);
}

// The hub-row segment kernel: one work item = kLongSeg consecutive nonzeros of a hub row (the row kernels' work list); every segment writes
// its partial row.  LOOP: a grid-stride loop over the work list (ctx->long_grid workgroups).  Otherwise one group per item over a grid that
// covers the list's capacity: the loop keeps every kernel argument alive across the row's walk, which in the GATv2 passes is more
// wave-uniform values than the bounds-checked row-pass instances have scalar registers for.
template <typename P, bool LOOP>
__global__ __launch_bounds__(kBlock) void attn_segments_kernel(const int2* __restrict__ items, const int* __restrict__ item_count, int capacity,
                                                               const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                               typename P::Args a, double* partials, int64_t pitch) {
    constexpr int LPR = P::lpr;
    constexpr int GROUPS = kBlock / LPR;
    const int tid = threadIdx.x;
    const int lig = tid % LPR;
    int count = *item_count;
    if (count > capacity) count = capacity;
    const int ngroups = (int)gridDim.x * GROUPS;
    int first = (int)blockIdx.x * GROUPS + tid / LPR;
    if constexpr (LPR == 64) first = __builtin_amdgcn_readfirstlane(first);
    for (int it = first; it < count; it += ngroups) {
        const int2 item = items[it];
        int rbeg = rowptr[item.x], rend = rowptr[item.x + 1], seg = item.y;
        int64_t row = item.x;
        if constexpr (LPR == 64) {
            rbeg = __builtin_amdgcn_readfirstlane(rbeg);
            rend = __builtin_amdgcn_readfirstlane(rend);
            seg = __builtin_amdgcn_readfirstlane(seg);
            row = __builtin_amdgcn_readfirstlane(item.x);
        }
        const int beg = rbeg + seg * kLongSeg;
        const int end = (beg + kLongSeg < rend) ? beg + kLongSeg : rend;
        P::run(row, beg, end, colidx, a, HNH_FUSED_OUT_OVERWRITE, lig, partials + (int64_t)it * pitch);
        if constexpr (!LOOP) break;  // one item per group
    }
}

// Out[row, 0 : f) += the row's segments' partial rows, front to back: one workgroup per hub row, one thread per column
__global__ __launch_bounds__(kBlock) void attn_grad_reduce_kernel(const int4* __restrict__ hub_rows, const int* __restrict__ counts, int capacity_rows,
                                                                  const double* __restrict__ partials, int64_t pitch, double* __restrict__ Out,
                                                                  int64_t ld_out, int f) {
    int nrows = counts[1];
    if (nrows > capacity_rows) nrows = capacity_rows;
    for (int e = (int)blockIdx.x; e < nrows; e += (int)gridDim.x) {
        const int4 h = hub_rows[e];  // (row, first item, segments, -)
        for (int c = threadIdx.x; c < f; c += kBlock) {
            const double* p = partials + (int64_t)h.y * pitch + c;
            double sum = 0.0;
#pragma unroll 8
            for (int s = 0; s < h.z; s++) sum += p[(int64_t)s * pitch];
            Out[(int64_t)h.x * ld_out + c] += sum;
        }
    }
}

__global__ __launch_bounds__(kBlock) void attn_grad_zero_rows_kernel(double* __restrict__ Out, int64_t ld_out, int64_t rows, int f) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, total = rows * f;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) Out[(i / f) * ld_out + i % f] = 0.0;
}

struct AttnRowState {  // what a forward pass keeps per row
    double* lse;
    double* Out;
    double* row_max;
    double* row_sum;
    double* relu_dst;
    int64_t ld_out, relu_ld;
    int f;
};

// Where a backward pass's results go: dst[row, 0 : width) is columns [col, col + width) of a hub row's partial rows, added up in segment
// order; the same list names what HNH_FUSED_OUT_OVERWRITE zeroes in a block without nonzeros.  A forward pass has none.
struct AttnSums {
    struct Sum {
        int64_t col;
        double* dst;
        int64_t ld;
        int width;
    } s[2];
    int n = 0;
    void add(int64_t col, double* dst, int64_t ld, int width) { s[n++] = Sum{col, dst, ld, width}; }
};

// One launch of a pass's instance P over the rows' pieces [beg_ptr, end_ptr); with run_long the hub rows, once per pass and over their whole
// length: segments with partial rows of `pitch` doubles, then the ordered sums.  WHOLE and LOOP as in the kernels above.
template <typename P, bool WHOLE, bool LOOP>
int attn_launch(hnh_ctx* ctx, hipStream_t st, const LongCtl& lc, int64_t rows, const int32_t* rowptr, const int32_t* beg_ptr, const int32_t* end_ptr,
                const int32_t* colidx, const typename P::Args& a, unsigned flags, bool run_long, int64_t pitch, const AttnSums& sums) {
    constexpr int GROUPS = kBlock / P::lpr;
    const int64_t blocks = (rows + GROUPS - 1) / GROUPS;
    if (blocks <= 0) return HNH_OK;
    if (blocks > 0x7fffffffLL) return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, "too many rows for one launch");
    if (lc.enabled) flags |= kInternalSplitLong | ((unsigned)(lc.threshold / 64) << kLongRowShift);
    const size_t lds_pad = lc.lds_pad <= 48 * 1024 ? lc.lds_pad : 0;
    hipLaunchKernelGGL((attn_rows_kernel<P, WHOLE>), dim3((unsigned)blocks), dim3(kBlock), lds_pad, st, rows, rowptr, beg_ptr, end_ptr, colidx, a, flags);
    if (int rc = hnh::check_hip(ctx, hipGetLastError(), "attn_rows_kernel launch")) return rc;
    if constexpr (!WHOLE) {
        if (lc.enabled && run_long) {
            const int seg_blocks = LOOP ? ctx->long_grid : (lc.capacity + GROUPS - 1) / GROUPS;  // (one group per item of the list)
            hipLaunchKernelGGL((attn_segments_kernel<P, LOOP>), dim3((unsigned)(seg_blocks > 0 ? seg_blocks : 1)), dim3(kBlock), 0, st, lc.items, lc.count,
                               lc.capacity, rowptr, colidx, a, lc.partials, pitch);
            if (int rc = hnh::check_hip(ctx, hipGetLastError(), "attn_segments_kernel launch")) return rc;
            for (int i = 0; i < sums.n; i++) {
                const AttnSums::Sum& s = sums.s[i];
                hipLaunchKernelGGL(attn_grad_reduce_kernel, dim3(2048), dim3(kBlock), 0, st, lc.hub_rows, lc.count, lc.capacity_rows, lc.partials + s.col,
                                   pitch, s.dst, s.ld, s.width);
                if (int rc = hnh::check_hip(ctx, hipGetLastError(), "attn_grad_reduce_kernel launch")) return rc;
            }
        }
    }
    return HNH_OK;
}

// The head of a pass's dispatcher, in front of what is the family's own: the arguments are there, the flags are the pass's (a forward pass
// takes the finish, its activation and its addend), the head width is within the family's limit.  The caller goes on with `rows == 0`.
inline int attn_dispatch_head(hnh_ctx* ctx, const hnh_csr_block* b, bool have_args, int f, int max_f, const char* max_f_name, bool forward,
                              unsigned flags, const hnh_csr_window* win, const char* who) {
    if (!b || !have_args) return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": null block or arguments");
    if (int rc = check_common(ctx, b->rows, f, who)) return rc;
    if (flags & ~(HNH_FUSED_OUT_OVERWRITE | (forward ? (HNH_ATTN_FINISH | kAttnActMask | HNH_ATTN_ADDEND) : 0u)))
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": unknown flag");
    if (int rc = check_attn_act_flags(ctx, flags, who)) return rc;
    if (f > max_f)
        return hnh::fail(ctx, HNH_ERR_UNSUPPORTED, std::string(who) + ": head width " + std::to_string(f) + " beyond the limit of " +
                                                       std::to_string(max_f) + " (" + max_f_name + ")");
    if (forward && (flags & HNH_ATTN_FINISH) && win != nullptr && !win->last)
        return hnh::fail(ctx, HNH_ERR_INVALID, std::string(who) + ": the finish belongs to the last window");
    return HNH_OK;
}

// A block without nonzeros (rowptr == nullptr), behind the family's checks of its outputs.  A forward pass (`state`, with the kernels' flags)
// resets and finishes every row; a backward pass zeroes what it would have overwritten.  (Defined in hnh_attn_additive_kernels.hpp, next to
// the forward passes' attn_add_empty_rows_kernel.)
int attn_dispatch_no_nonzeros(hnh_ctx* ctx, hipStream_t st, const hnh_csr_block* b, unsigned kflags, const AttnRowState* state, const AttnSums& sums,
                              const char* who);

// The tail of a pass's dispatcher, behind its argument checks: the block's structure plan; the hub rows' work list with a partial result
// of `pitch` doubles per segment (pitch 0: hub rows are walked whole, as the forward passes do: a row's scores are combined in row order,
// never by segments); the LDS pad; then ONE launch for the selected window(s) or an unsplit block, or one per Infinity-Cache panel of the
// `gather_w` wide gathered operand.  launch(lc, beg_ptr, end_ptr, flags, run_long) is the pass's instance.
template <typename Launch>
int attn_dispatch_tail(hnh_ctx* ctx, hipStream_t st, int stream, const hnh_csr_block* b, const hnh_csr_window* win, int f, bool w2, int64_t pitch,
                       int gather_w, unsigned flags, const char* who, Launch&& launch) {
    const int64_t rows = b->rows, nnz = b->nnz;
    const int32_t* rowptr = b->rowptr;
    if (int rc = adopt_plan(ctx, b->plan, rows, nnz, rowptr, b->col_idx)) return rc;
    LongCtl lc;
    if (pitch > 0) {
        if (int rc = prepare_long(ctx, st, stream, rows, rowptr, nnz, b->max_row_nnz, pitch, &lc, win == nullptr || win->last != 0, b->plan)) return rc;
        if (lc.enabled && lc.items != nullptr) {  // this pass has hub rows: every segment needs its partial result (no atomics here)
            if (lc.partials == nullptr)
                if (int rc = partial_scratch(ctx, st, stream, (size_t)lc.capacity, pitch, &lc)) return rc;
            if (lc.partials == nullptr || lc.partial_items < lc.capacity)
                return hnh::fail(ctx, HNH_ERR_NOMEM, std::string(who) + ": the hub rows' partial rows exceed HNH_HUB_SCRATCH_MB");
        }
    }
    if (!lc.enabled || ctx->row_waves_cap > 0) {
        Shape s = pick_shape(f, w2);
        lc.lds_pad = row_occupancy_pad(ctx, s, rows, nnz, b->max_row_nnz);
    }
    if (win != nullptr) {
        const int32_t* beg_ptr = win->beg ? win->beg : rowptr;
        const int32_t* end_ptr = win->end ? win->end : rowptr + 1;
        return launch(lc, beg_ptr, end_ptr, flags, win->last != 0);
    }
    const int panels = (!lc.enabled || ctx->panels_with_hubs) ? panel_count(ctx, b->cols, gather_w) : 1;
    if (panels > 1) {
        int32_t* split = nullptr;
        if (int rc = panel_split_rows(ctx, st, stream, b->plan, rows, b->cols, rowptr, b->col_idx, panels, &split)) return rc;
        for (int q = 0; q < panels; q++) {
            const int32_t* beg_ptr = (q == 0) ? rowptr : split + (size_t)(q - 1) * rows;
            const int32_t* end_ptr = (q == panels - 1) ? rowptr + 1 : split + (size_t)q * rows;
            unsigned fq = flags;
            if (q > 0) fq &= ~HNH_FUSED_OUT_OVERWRITE;     // later panels continue the rows the first one started
            if (q < panels - 1) fq &= ~kInternalEpilogue;  // the last panel finishes them (only a forward pass sets it)
            if (int rc = launch(lc, beg_ptr, end_ptr, fq, q == panels - 1)) return rc;
        }
        return HNH_OK;
    }
    return launch(lc, rowptr, rowptr + 1, flags, true);
}

}  // namespace
