#include <functional>
#include "sparse_kernels.hpp"

// SDDMM of operands up to this many columns goes through the nonzero-balanced COO kernel (StandardKernel::sddmm_local)
static constexpr int64_t kCooSddmmMaxWidth = 16;

// StandardKernel::sddmm_local — sparse_kernels.cpp:13-57 of the reference:
//   values[i] += <Arow(row_idx[i]), Brow(col_idx[i])>, with A and B swapped when the block is stored
//   transposed (:29-37); a null block is a no-op (:25-27); always reports 0 nonzeros (:23,56).
size_t StandardKernel::sddmm_local(SpmatLocal& S, DenseMatrix& A, DenseMatrix& B, int block, int offset) {
    (void)offset;  // ignored by the reference as well (15D_sparse_shift.hpp:245 TODO)
    if (A.cols() != B.cols()) hnh::fatal("Error, SDDMM operands must have the same number of columns!");
    size_t processed = 0;
    CSRLocal* blk = S.csr_blocks[block];
    if (blk == nullptr || blk->num_coords == 0) return processed;
    double* Xptr = (blk->transpose ? B.data() : A.data()) + blk->part_first_row() * A.cols();  // (a row range reads its own rows of the row operand)
    double* Yptr = blk->transpose ? A.data() : B.data();
    CSRHandle* active = blk->getActive();
    hnh::World* w = S.world;
    begin(w);
    hnh_csr_window win;
    const hnh_csr_block desc = blk->block_args();
    const unsigned fresh = blk->values_fresh ? HNH_FUSED_VALUES_OVERWRITE : 0u;  // first visit: store instead of read-add-store
    // (a lent destination: the products scale .* dots go straight into the caller's result vector, CSRLocal::sddmm_dst)
    double* dst = blk->sddmm_dst ? blk->sddmm_dst : active->values;
    const double* scale = blk->sddmm_dst ? blk->sddmm_scale : nullptr;
    if (blk->window_args(&win)) {  // one column range of the block (the schedule walks them as their data arrives)
        w->check(w->be->hnh_sddmm_csr_ps(w->ctx, &desc, dst, scale, Xptr, Yptr, (int)A.cols(), fresh, &win, HNH_STREAM_COMPUTE), "hnh_sddmm_csr_ps");
        end(w);
        return processed;
    }
    if (A.cols() <= kCooSddmmMaxWidth && !fresh && scale == nullptr && blk->range_sel < 0) {  // (the COO kernel accumulates: first visits take the storing CSR pass)
        // narrow operands, ACCUMULATING visit (the travelling blocks of 15d_sparse / 2.5D dense after their first step): several sparse
        // rows share a wave in the row kernel and the wave runs as long as its longest row; the COO kernel deals nonzeros out evenly
        // instead.  Re-measured in round 5 with the line-granular row loop (config-2 size, profiles/r05_kbench_narrow.log): accumulating
        // row pass 2.062 / 2.132 ms at R = 8 / 16 against 2.025 / 2.055 ms here — the row loop already reads the value line with the
        // index line and writes whole lines, what it cannot shed is the longest-row effect — so these two widths stay on this kernel
        // (1.8 % / 3.7 %); STORING visits (every first visit) are faster through the row pass (1.925 / 2.003 ms) and never come here; from
        // R = 32 the row pass wins either way (3.825 vs 3.978 ms)
        const int32_t* row_idx = blk->ensure_row_idx(HNH_STREAM_COMPUTE);
        w->check(w->be->hnh_sddmm_coo(w->ctx, blk->num_coords, row_idx, active->col_idx, active->values, Xptr, Yptr, (int)A.cols(),
                                      HNH_STREAM_COMPUTE),
                 "hnh_sddmm_coo");
        end(w);
        return processed;
    }
    w->check(w->be->hnh_sddmm_csr_ps(w->ctx, &desc, dst, scale, Xptr, Yptr, (int)A.cols(), fresh, nullptr, HNH_STREAM_COMPUTE), "hnh_sddmm_csr_ps");
    end(w, profile ? w->be->hnh_panel_count(w->ctx, desc.rows, desc.nnz, desc.cols, (int)A.cols(), desc.max_row_nnz) : 1);
    return processed;
}

// StandardKernel::spmm_local — sparse_kernels.cpp:59-127: C += S_blk * X with alpha = beta = 1.
size_t StandardKernel::spmm_local(SpmatLocal& S, DenseMatrix& A, DenseMatrix& B, MatMode mode, int block) {
    size_t processed = 0;
    CSRLocal* blk = S.csr_blocks[block];
    if (blk == nullptr) return processed;
    if (mode == Amat && blk->transpose) hnh::fatal("Error, local matrix is transposed, can't perform SpmmA");
    else if (mode == Bmat && !blk->transpose) hnh::fatal("Error, local matrix is not transposed, can't perform SpmmB");
    CSRHandle* active = blk->getActive();
    hnh::World* w = S.world;
    const double* X = (mode == Amat) ? B.data() : A.data();
    double* Out = ((mode == Amat) ? A.data() : B.data()) + blk->part_first_row() * A.cols();  // (a row part writes its own rows of the output)
    if (blk->num_coords == 0) {  // nothing to multiply; fresh output rows still have to hold zeros afterwards
        if (blk->out_fresh) {
            const hnh_csr_block d0 = blk->block_args();
            w->check(w->be->hnh_fill_f64(w->ctx, Out, d0.rows * A.cols(), 0.0, HNH_STREAM_COMPUTE), "hnh_fill_f64");
        }
        return processed;
    }
    const double* vals = blk->spmm_values ? blk->spmm_values : active->values;  // (lent: the caller's SValues slice, read in place)
    begin(w);
    hnh_csr_window win;
    const hnh_csr_block desc = blk->block_args();
    if (blk->window_args(&win)) {
        w->check(w->be->hnh_spmm_csr_p(w->ctx, &desc, vals, X, Out, (int)A.cols(), &win, HNH_STREAM_COMPUTE), "hnh_spmm_csr_p");
        end(w);
        return processed;
    }
    // (a fresh output: the selected rows of Out are STORED, not added to — the staging rows of the mesh reduce-scatter are written once)
    w->check(w->be->hnh_spmm_csr_pf(w->ctx, &desc, vals, X, Out, (int)A.cols(), blk->out_fresh ? HNH_FUSED_OUT_OVERWRITE : 0u, nullptr, HNH_STREAM_COMPUTE),
             "hnh_spmm_csr_pf");
    end(w, profile ? w->be->hnh_panel_count(w->ctx, desc.rows, desc.nnz, desc.cols, (int)A.cols(), desc.max_row_nnz) : 1);
    return processed;
}

// One pass for the sddmm/spmm pair of 15D_dense_shift.hpp:203-217 (block not transposed: approach 2).
size_t StandardKernel::fused_local(SpmatLocal& S, DenseMatrix& A, DenseMatrix& B, DenseMatrix& Out, int block, unsigned flags,
                                   const hnh_fused_extras* extras) {
    if (A.cols() != B.cols() || Out.cols() != A.cols()) hnh::fatal("Error, fused operands must have the same number of columns!");
    if ((flags & HNH_FUSED_LEAKY_RELU) && !extras) hnh::fatal("Error, HNH_FUSED_LEAKY_RELU needs extras!");
    CSRLocal* blk = S.csr_blocks[block];
    hnh::World* w = S.world;
    if (blk == nullptr || blk->num_coords == 0) {  // nothing to multiply; the flags' contract and the row epilogue still apply
        if (flags & HNH_FUSED_OUT_OVERWRITE) Out.setZero();  // "treat Out as zero on entry": it must not keep stale rows
        row_epilogue(w, A, Out, extras);
        return 0;
    }
    if (blk->transpose) hnh::fatal("Error, local matrix is transposed, can't perform the fused SDDMM+SpMM");
    CSRHandle* active = blk->getActive();
    begin(w);
    hnh_csr_window win;
    const hnh_csr_block desc = blk->block_args();
    if (blk->window_args(&win)) {
        if (wants_epilogue(extras) && !win.last) hnh::fatal("Error, the row epilogue belongs to the block's last window!");
        w->check(w->be->hnh_fused_sddmm_spmm_csr_p(w->ctx, &desc, active->values, nullptr, A.data(), B.data(), Out.data(), (int)A.cols(), flags, extras,
                                                   &win, HNH_STREAM_COMPUTE),
                 "hnh_fused_sddmm_spmm_csr_p");
        end(w);
        return 0;
    }
    w->check(w->be->hnh_fused_sddmm_spmm_csr_p(w->ctx, &desc, active->values, nullptr, A.data(), B.data(), Out.data(), (int)A.cols(), flags, extras,
                                               nullptr, HNH_STREAM_COMPUTE),
             "hnh_fused_sddmm_spmm_csr_p");
    end(w, profile ? w->be->hnh_panel_count(w->ctx, desc.rows, desc.nnz, desc.cols, (int)A.cols(), desc.max_row_nnz) : 1);
    return 0;
}

bool KernelImplementation::softmax_local(SpmatLocal& S, DenseMatrix& A, DenseMatrix& B, DenseMatrix& Out, int block, unsigned flags,
                                         const hnh_attn_state& state, bool finish) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->softmax_block(S, A, B, Out, block, flags, state, finish);
}

// The softmax instance of the fused pass (include/hnh_attention.h), next to fused_local: same block and window handling, the finish
// belongs to the pass's last call (win.last when windows are selected).
bool StandardKernel::softmax_block(SpmatLocal& S, DenseMatrix& A, DenseMatrix& B, DenseMatrix& Out, int block, unsigned flags,
                                   const hnh_attn_state& state, bool finish) {
    hnh::World* w = S.world;
    if (w->be->hnh_attn_softmax_csr_p == nullptr)
        throw hnh::Error(std::string("Error, softmax attention needs the kernel hnh_attn_softmax_csr_p, which the kernel library ") + w->be->path +
                         " does not export (include/hnh_attention.h)");
    if (A.cols() != B.cols() || Out.cols() != A.cols()) hnh::fatal("Error, fused operands must have the same number of columns!");
    if (Out.rows() != A.rows()) hnh::fatal("Error, the softmax pass needs an output of the row operand's shape!");
    CSRLocal* blk = S.csr_blocks[block];
    const unsigned f = flags | (finish ? HNH_ATTN_FINISH : 0u);
    if (blk == nullptr || blk->num_coords == 0) {  // nothing to multiply; the state reset and the finish still apply
        hnh_csr_block none = {};
        none.rows = Out.rows();
        none.cols = -1;
        w->check(w->be->hnh_attn_softmax_csr_p(w->ctx, &none, nullptr, A.data(), B.data(), Out.data(), (int)A.cols(), f & ~HNH_FUSED_VALUES_OVERWRITE,
                                               &state, nullptr, HNH_STREAM_COMPUTE),
                 "hnh_attn_softmax_csr_p");
        return true;
    }
    if (blk->transpose) hnh::fatal("Error, local matrix is transposed, can't perform the fused SDDMM+SpMM");
    begin(w);
    hnh_csr_window win;
    const hnh_csr_block desc = blk->block_args();
    const bool windowed = blk->window_args(&win);
    if (windowed && finish && !win.last) hnh::fatal("Error, the softmax finish belongs to the block's last window!");
    w->check(w->be->hnh_attn_softmax_csr_p(w->ctx, &desc, blk->getActive()->values, A.data(), B.data(), Out.data(), (int)A.cols(), f, &state,
                                           windowed ? &win : nullptr, HNH_STREAM_COMPUTE),
             "hnh_attn_softmax_csr_p");
    end(w, (profile && !windowed) ? w->be->hnh_panel_count(w->ctx, desc.rows, desc.nnz, desc.cols, (int)A.cols(), desc.max_row_nnz) : 1);
    return true;
}

// The block and window handling that the attention passes share around their backend call `call(descriptor, window)`, `pass` in the complaints.
// An absent or empty block still gets the call, with the output's rows alone: an overwrite's zeroing, the state reset and the forward finish
// apply to it too.  Otherwise the call runs between begin() and end(launches), the profile's event pair, with the panel count of a `width`
// wide operand when no window is selected.  finish_text != nullptr: the call finishes a forward pass, which belongs to the block's last window.
template <typename Call, typename Begin, typename End>
static void attn_block_call(SpmatLocal& S, int block, int64_t rows, const std::string& pass, const char* finish_text, int width, bool profile,
                            Call&& call, Begin&& begin, End&& end) {
    hnh::World* w = S.world;
    CSRLocal* blk = S.csr_blocks[block];
    if (blk == nullptr || blk->num_coords == 0) {
        hnh_csr_block none = {};
        none.rows = rows;
        none.cols = -1;
        call(none, nullptr);
        return;
    }
    if (blk->transpose) hnh::fatal("Error, local matrix is transposed, can't perform " + pass);
    begin();
    hnh_csr_window win;
    const hnh_csr_block desc = blk->block_args();
    if (desc.rows != rows) hnh::fatal("Error, " + pass + " needs an output of the block's rows!");
    const bool windowed = blk->window_args(&win);
    if (windowed && finish_text != nullptr && !win.last) hnh::fatal(finish_text);
    call(desc, windowed ? &win : nullptr);
    end((profile && !windowed) ? w->be->hnh_panel_count(w->ctx, desc.rows, desc.nnz, desc.cols, width, desc.max_row_nnz) : 1);
}

bool KernelImplementation::attn_grad_local(SpmatLocal& S, int block, const hnh_attn_grad& args, bool column_side, unsigned flags, int64_t rows) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_grad_block(S, block, args, column_side, flags, rows);
}

// The two passes of the fused attention backward (include/hnh_attn_grad.h), next to fused_local: same block and window handling.
bool StandardKernel::attn_grad_block(SpmatLocal& S, int block, const hnh_attn_grad& args, bool column_side, unsigned flags, int64_t rows) {
    hnh::World* w = S.world;
    auto fn = column_side ? w->be->hnh_attn_grad_col_csr_p : w->be->hnh_attn_grad_row_csr_p;
    const char* name = column_side ? "hnh_attn_grad_col_csr_p" : "hnh_attn_grad_row_csr_p";
    if (fn == nullptr)
        throw hnh::Error(std::string("Error, the fused attention backward needs the kernel ") + name + ", which the kernel library " + w->be->path +
                         " does not export (include/hnh_attn_grad.h)");
    attn_block_call(S, block, rows, "the fused attention backward", nullptr, column_side ? 2 * args.f : args.f, profile,
                    [&](const hnh_csr_block& d, const hnh_csr_window* win) { w->check(fn(w->ctx, &d, &args, flags, win, HNH_STREAM_COMPUTE), name); },
                    [&] { begin(w); }, [&](long launches) { end(w, launches); });
    return true;
}

bool KernelImplementation::attn_additive_local(SpmatLocal& S, int block, const hnh_attn_add& args, int pass, unsigned flags, int64_t rows, bool finish) {
    return attn_additive_local(S, block, args, pass, flags, rows, finish, nullptr);
}

bool KernelImplementation::attn_additive_local(SpmatLocal& S, int block, const hnh_attn_add& args, int pass, unsigned flags, int64_t rows, bool finish,
                                               const hnh_attn_drop* drop) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_additive_block(S, block, args, pass, flags, rows, finish, drop);
}

// The three passes of the additive-score attention (include/hnh_attn_additive.h), next to attn_grad_block: same block and window handling.
bool StandardKernel::attn_additive_block(SpmatLocal& S, int block, const hnh_attn_add& args, int pass, unsigned flags, int64_t rows, bool finish) {
    return attn_additive_block(S, block, args, pass, flags, rows, finish, nullptr);
}

// ... and with `drop` their DROP instances (include/hnh_attn_dropout.h): the same calls with one more argument.
bool StandardKernel::attn_additive_block(SpmatLocal& S, int block, const hnh_attn_add& args, int pass, unsigned flags, int64_t rows, bool finish,
                                         const hnh_attn_drop* drop) {
    hnh::World* w = S.world;
    auto plain = pass == 0 ? w->be->hnh_attn_add_fwd_csr_p : (pass == 1 ? w->be->hnh_attn_add_row_csr_p : w->be->hnh_attn_add_col_csr_p);
    auto masked = pass == 0 ? w->be->hnh_attn_drop_fwd_csr_p : (pass == 1 ? w->be->hnh_attn_drop_row_csr_p : w->be->hnh_attn_drop_col_csr_p);
    const char* name = drop ? (pass == 0 ? "hnh_attn_drop_fwd_csr_p" : (pass == 1 ? "hnh_attn_drop_row_csr_p" : "hnh_attn_drop_col_csr_p"))
                            : (pass == 0 ? "hnh_attn_add_fwd_csr_p" : (pass == 1 ? "hnh_attn_add_row_csr_p" : "hnh_attn_add_col_csr_p"));
    if (drop ? masked == nullptr : plain == nullptr)
        throw hnh::Error(std::string("Error, the additive attention score needs the kernel ") + name + ", which the kernel library " + w->be->path +
                         " does not export (" + (drop ? "include/hnh_attn_dropout.h" : "include/hnh_attn_additive.h") + ")");
    auto fn = [&](hnh_ctx* ctx, const hnh_csr_block* b, const hnh_attn_add* a, unsigned fl, const hnh_csr_window* win, int stream) {
        return drop ? masked(ctx, b, a, drop, fl, win, stream) : plain(ctx, b, a, fl, win, stream);
    };
    const unsigned f = flags | ((pass == 0 && finish) ? HNH_ATTN_FINISH : 0u);
    const char* finish_text = (pass == 0 && finish) ? "Error, the additive forward finish belongs to the block's last window!" : nullptr;
    attn_block_call(S, block, rows, "the additive attention pass", finish_text, (pass == 2 || drop) ? HNH_ATTN_ADD_PACKED_WIDTH(args.f) : HNH_ATTN_ADD_SCORED_WIDTH(args.f),
                    profile, [&](const hnh_csr_block& d, const hnh_csr_window* win) { w->check(fn(w->ctx, &d, &args, f, win, HNH_STREAM_COMPUTE), name); },
                    [&] { begin(w); }, [&](long launches) { end(w, launches); });
    return true;
}

bool KernelImplementation::attn_v2_local(SpmatLocal& S, int block, const hnh_attn_v2& args, int pass, unsigned flags, int64_t rows, bool finish) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_v2_block(S, block, args, pass, flags, rows, finish);
}

// The three sparse passes of the GATv2 attention (include/hnh_attn_v2.h), next to attn_additive_block: same block and window handling.
bool StandardKernel::attn_v2_block(SpmatLocal& S, int block, const hnh_attn_v2& args, int pass, unsigned flags, int64_t rows, bool finish) {
    hnh::World* w = S.world;
    auto fn = pass == 0 ? w->be->hnh_attn_v2_fwd_csr_p : (pass == 1 ? w->be->hnh_attn_v2_row_csr_p : w->be->hnh_attn_v2_col_csr_p);
    const char* name = pass == 0 ? "hnh_attn_v2_fwd_csr_p" : (pass == 1 ? "hnh_attn_v2_row_csr_p" : "hnh_attn_v2_col_csr_p");
    if (fn == nullptr)
        throw hnh::Error(std::string("Error, the gatv2 attention score needs the kernel ") + name + ", which the kernel library " + w->be->path +
                         " does not export (include/hnh_attn_v2.h)");
    const unsigned f = flags | ((pass == 0 && finish) ? HNH_ATTN_FINISH : 0u);
    const char* finish_text = (pass == 0 && finish) ? "Error, the gatv2 forward finish belongs to the block's last window!" : nullptr;
    attn_block_call(S, block, rows, "the gatv2 attention pass", finish_text, pass == 2 ? HNH_ATTN_GRAD_PACKED_WIDTH(args.f, 1) : args.f, profile,
                    [&](const hnh_csr_block& d, const hnh_csr_window* win) { w->check(fn(w->ctx, &d, &args, f, win, HNH_STREAM_COMPUTE), name); },
                    [&] { begin(w); }, [&](long launches) { end(w, launches); });
    return true;
}

bool KernelImplementation::attn_qkv_local(SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_qkv_block(S, block, args, pass, flags, rows, finish);
}

// The three sparse passes of the query/key/value attention (include/hnh_attn_qkv.h), next to attn_v2_block: same block and window handling;
// the gathered width is the packed operand's of the pass.  `biased`: the entry points of include/hnh_attn_edge.h, which take the block's
// slice of the bias vector behind the arguments; `graded`: those of include/hnh_attn_edge_grad.h (the backward passes alone), which also
// take the block's slice of the bias's gradient and `accumulate`; every overload of attn_qkv_block is this one function.
static bool attn_qkv_call(StandardKernel& k, SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish,
                          bool biased, const double* bias, const std::function<void()>& begin, const std::function<void(long)>& end,
                          bool graded = false, double* dbias = nullptr, bool accumulate = false) {
    hnh::World* w = S.world;
    const hnh::Backend* be = w->be;
    auto plain = pass == 0 ? be->hnh_attn_qkv_fwd_csr_p : (pass == 1 ? be->hnh_attn_qkv_row_csr_p : be->hnh_attn_qkv_col_csr_p);
    auto with_bias = pass == 0 ? be->hnh_attn_qkv_bias_fwd_csr_p : (pass == 1 ? be->hnh_attn_qkv_bias_row_csr_p : be->hnh_attn_qkv_bias_col_csr_p);
    if (graded) {
        if (pass != 1 && pass != 2) hnh::fatal("Error, the edge bias's gradient belongs to the backward passes!");
        auto with_grad = pass == 1 ? be->hnh_attn_qkv_bias_grad_row_csr_p : be->hnh_attn_qkv_bias_grad_col_csr_p;
        const char* gname = pass == 1 ? "hnh_attn_qkv_bias_grad_row_csr_p" : "hnh_attn_qkv_bias_grad_col_csr_p";
        if (with_grad == nullptr)
            throw hnh::Error(std::string("Error, the transformer attention score with a learned edge bias needs the kernel ") + gname +
                             ", which the kernel library " + be->path + " does not export (include/hnh_attn_edge_grad.h)");
        attn_block_call(S, block, rows, "the transformer attention pass with a learned edge bias", nullptr, HNH_ATTN_GRAD_PACKED_WIDTH(args.f, pass == 2 ? 1 : 0),
                        k.profile,
                        [&](const hnh_csr_block& d, const hnh_csr_window* win) {
                            w->check(with_grad(w->ctx, &d, &args, bias, dbias, accumulate ? 1 : 0, flags, win, HNH_STREAM_COMPUTE), gname);
                        },
                        begin, end);
        return true;
    }
    const std::string name = std::string(biased ? "hnh_attn_qkv_bias_" : "hnh_attn_qkv_") + (pass == 0 ? "fwd" : (pass == 1 ? "row" : "col")) + "_csr_p";
    if (biased ? with_bias == nullptr : plain == nullptr)
        throw hnh::Error(std::string("Error, the transformer attention score") + (biased ? " with an edge bias" : "") + " needs the kernel " + name +
                         ", which the kernel library " + be->path + " does not export (" + (biased ? "include/hnh_attn_edge.h" : "include/hnh_attn_qkv.h") + ")");
    const unsigned f = flags | ((pass == 0 && finish) ? HNH_ATTN_FINISH : 0u);
    const char* finish_text = (pass == 0 && finish) ? "Error, the transformer forward finish belongs to the block's last window!" : nullptr;
    attn_block_call(S, block, rows, biased ? "the transformer attention pass with an edge bias" : "the transformer attention pass", finish_text,
                    HNH_ATTN_GRAD_PACKED_WIDTH(args.f, pass == 2 ? 1 : 0), k.profile,
                    [&](const hnh_csr_block& d, const hnh_csr_window* win) {
                        w->check(biased ? with_bias(w->ctx, &d, &args, bias, f, win, HNH_STREAM_COMPUTE) : plain(w->ctx, &d, &args, f, win, HNH_STREAM_COMPUTE),
                                 name.c_str());
                    },
                    begin, end);
    return true;
}

bool StandardKernel::attn_qkv_block(SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish) {
    return attn_qkv_call(*this, S, block, args, pass, flags, rows, finish, false, nullptr, [&] { begin(S.world); }, [&](long n) { end(S.world, n); });
}

bool KernelImplementation::attn_qkv_local(SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish,
                                          const double* bias) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_qkv_block(S, block, args, pass, flags, rows, finish, bias);
}

bool StandardKernel::attn_qkv_block(SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish,
                                    const double* bias) {
    return attn_qkv_call(*this, S, block, args, pass, flags, rows, finish, true, bias, [&] { begin(S.world); }, [&](long n) { end(S.world, n); });
}

bool KernelImplementation::attn_qkv_local(SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish,
                                          const double* bias, double* dbias, bool accumulate) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_qkv_block(S, block, args, pass, flags, rows, finish, bias, dbias, accumulate);
}

bool StandardKernel::attn_qkv_block(SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish,
                                    const double* bias, double* dbias, bool accumulate) {
    return attn_qkv_call(*this, S, block, args, pass, flags, rows, finish, true, bias, [&] { begin(S.world); }, [&](long n) { end(S.world, n); }, true, dbias,
                         accumulate);
}

bool KernelImplementation::attn_coef_local(SpmatLocal& S, int block, const hnh_attn_coef& args, int64_t rows, const hnh_attn_drop* drop) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_coef_block(S, block, args, rows, drop);
}

// The export of the attention coefficients (include/hnh_attn_coef.h), next to attn_v2_block: same block and window handling; the values go
// where an SDDMM's would (a lent slice of the caller's vector, or the block's own array).
bool StandardKernel::attn_coef_block(SpmatLocal& S, int block, const hnh_attn_coef& args, int64_t rows, const hnh_attn_drop* drop) {
    hnh::World* w = S.world;
    const char* name = "hnh_attn_coef_csr_p";
    if (w->be->hnh_attn_coef_csr_p == nullptr)
        throw hnh::Error(std::string("Error, the export of the attention coefficients needs the kernel ") + name + ", which the kernel library " +
                         w->be->path + " does not export (include/hnh_attn_coef.h)");
    CSRLocal* blk = S.csr_blocks[block];
    double* dst = blk == nullptr ? nullptr : (blk->sddmm_dst ? blk->sddmm_dst : blk->getActive()->values);
    attn_block_call(S, block, rows, "the attention-coefficient export", nullptr,
                    args.score == HNH_ATTN_COEF_ADDITIVE ? HNH_ATTN_COEF_PAIR_WIDTH : args.f, profile,
                    [&](const hnh_csr_block& d, const hnh_csr_window* win) {
                        w->check(w->be->hnh_attn_coef_csr_p(w->ctx, &d, dst, &args, drop, 0u, win, HNH_STREAM_COMPUTE), name);
                    },
                    [&] { begin(w); }, [&](long launches) { end(w, launches); });
    return true;
}

void StandardKernel::begin(hnh::World* w) {
    if (!profile) return;
    if (evw_ != nullptr && evw_ != w) hnh::fatal("Error, a profiled StandardKernel belongs to one world!");
    evw_ = w;
    if (used_ == pairs_.size()) {
        if (used_ >= 4096) resolve_profile();  // (bounded: a very long profiled section reads its pairs now and reuses them)
        else pairs_.emplace_back(w->event_create(), w->event_create());
    }
    // A start event right behind a cross-stream wait is stamped when the stream's EARLIER work completes, not when the wait is satisfied
    // (measured: the two-half accumulator ring's 16 launches summed to 4.5 ms inside a 2.9 ms call, profiles/r06_job4_fusion1_rank_share.log):
    // the span would count the wait for a transfer as kernel time.  A dispatch cannot start before the wait is satisfied, so a tiny one
    // (8 bytes filled) goes in front of the start event: its end is the earliest moment the kernel could have started.
    if (!tick_) tick_ = w->dmalloc(8);
    w->memset0(tick_, 8, HNH_STREAM_COMPUTE);
    w->event_record(pairs_[used_].first, HNH_STREAM_COMPUTE);
}

void StandardKernel::end(hnh::World* w, long launches) {
    if (!profile) return;
    w->event_record(pairs_[used_].second, HNH_STREAM_COMPUTE);
    used_++;
    kernel_launches += launches;  // a row pass may run as several column-panel launches (hnh_panel_count)
}

void StandardKernel::resolve_profile() {
    if (used_ == 0) return;
    hnh::World* w = evw_;
    w->check(w->be->hnh_event_sync(w->ctx, pairs_[used_ - 1].second), "hnh_event_sync");  // (same stream: the last pair completes last)
    for (size_t k = 0; k < used_; k++) {
        float ms = 0.f;
        w->check(w->be->hnh_event_elapsed_ms(w->ctx, pairs_[k].first, pairs_[k].second, &ms), "hnh_event_elapsed_ms");
        kernel_ms += ms;
    }
    used_ = 0;
}

StandardKernel::~StandardKernel() {
    if (evw_) {
        for (auto& pr : pairs_) {
            evw_->event_destroy(pr.first);
            evw_->event_destroy(pr.second);
        }
        if (tick_) evw_->dfree(tick_);
    }
}
