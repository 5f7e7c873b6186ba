// What the dispatchers of the attention passes share (hnh_attn_grad_kernels.hpp, hnh_attn_additive_kernels.hpp and, through the latter,
// the DROP instances): host code only.  Included by the first of them, inside hnh_kernels.hip, whose plans, hub-row work lists, LDS pad
// and Infinity-Cache panels it drives; every pass keeps its own argument checks, its own kernel arguments and its own launcher.
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
