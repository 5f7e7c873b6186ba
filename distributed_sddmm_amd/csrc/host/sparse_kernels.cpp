#include "sparse_kernels.hpp"
#include <type_traits>

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
    CSRHandle* active = blk->getActive();  // (blk->spmm_values: null, or the lent per-nonzero weights of the SpMM half, lendFusedWeights)
    begin(w);
    hnh_csr_window win;
    const hnh_csr_block desc = blk->block_args();
    if (blk->window_args(&win)) {
        if (wants_epilogue(extras) && !win.last) hnh::fatal("Error, the row epilogue belongs to the block's last window!");
        w->check(w->be->hnh_fused_sddmm_spmm_csr_p(w->ctx, &desc, active->values, blk->spmm_values, A.data(), B.data(), Out.data(), (int)A.cols(), flags, extras,
                                                   &win, HNH_STREAM_COMPUTE),
                 "hnh_fused_sddmm_spmm_csr_p");
        end(w);
        return 0;
    }
    w->check(w->be->hnh_fused_sddmm_spmm_csr_p(w->ctx, &desc, active->values, blk->spmm_values, A.data(), B.data(), Out.data(), (int)A.cols(), flags, extras,
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
        throw hnh::Error(w->be->missing_kernel("softmax attention", "hnh_attn_softmax_csr_p"));
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

// The block and window handling round an attention pass's backend call `call(descriptor, window)`, `pass` in the complaints.
// An absent or empty block still gets the call, with the output's rows alone: an overwrite's zeroing, the state reset and the forward finish
// apply to it too.  Otherwise the call runs between begin() and end(launches), the profile's event pair, with the panel count of a `width`
// wide operand when no window is selected.  finish_text != nullptr: the call finishes a forward pass, which belongs to the block's last window.
template <typename Call>
void StandardKernel::attn_block_call(SpmatLocal& S, int block, int64_t rows, const std::string& pass, const char* finish_text, int width, Call&& call) {
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
    begin(w);
    hnh_csr_window win;
    const hnh_csr_block desc = blk->block_args();
    if (desc.rows != rows) hnh::fatal("Error, " + pass + " needs an output of the block's rows!");
    const bool windowed = blk->window_args(&win);
    if (windowed && finish_text != nullptr && !win.last) hnh::fatal(finish_text);
    call(desc, windowed ? &win : nullptr);
    end(w, (profile && !windowed) ? w->be->hnh_panel_count(w->ctx, desc.rows, desc.nnz, desc.cols, width, desc.max_row_nnz) : 1);
}

// ---- the attention passes' entry points (include/hnh_attn_grad.h, _additive.h, _dropout.h, _v2.h, _qkv.h, _edge.h, _edge_grad.h, _coef.h):
// one row each.  A further score is a further alternative of hnh::AttnPass::args, its rows here and its call in attn_block.
using hnh::AttnPass;
namespace {
enum Variant { PLAIN, DROP, BIAS, BIAS_GRAD };  // the plain entry point; with attention dropout; with an edge bias; ... and its gradient
Variant variant_of(const AttnPass& p) {
    if (p.family() == AttnPass::QKV) return p.dbias ? BIAS_GRAD : (p.bias ? BIAS : PLAIN);
    return (p.family() == AttnPass::ADDITIVE && p.drop) ? DROP : PLAIN;  // (the export takes `drop` as an argument of its one entry point)
}
// the gathered operand's width, which hnh_panel_count splits into column panels, from the head's f
int w_head(const AttnPass& p) { return std::visit([](const auto& a) { return (int)a.f; }, p.args); }
int w_pair(const AttnPass& p) { return 2 * w_head(p); }
int w_scored(const AttnPass& p) { return HNH_ATTN_ADD_SCORED_WIDTH(w_head(p)); }
int w_add_packed(const AttnPass& p) { return HNH_ATTN_ADD_PACKED_WIDTH(w_head(p)); }
int w_kv(const AttnPass& p) { return HNH_ATTN_GRAD_PACKED_WIDTH(w_head(p), 0); }
int w_packed(const AttnPass& p) { return HNH_ATTN_GRAD_PACKED_WIDTH(w_head(p), 1); }
int w_coef(const AttnPass& p) { return std::get<hnh_attn_coef>(p.args).score == HNH_ATTN_COEF_ADDITIVE ? HNH_ATTN_COEF_PAIR_WIDTH : w_head(p); }

struct AttnEntry {
    AttnPass::Family family;
    int pass;
    Variant variant;
    void* (*fn)(const hnh::Backend&);  // the Backend member
    const char* symbol;
    const char *feature, *label, *noun;  // "<feature> needs the kernel ..."; attn_block_call's complaints; "... has no <noun> (...)"
    const char* finish_text;             // of a forward pass's closing call, or none
    int (*width)(const AttnPass&);
};
#define HNH_ATTN_ENTRY(family, pass, variant, sym, ...) \
    {AttnPass::family, pass, variant, [](const hnh::Backend& be) { return (void*)be.sym; }, #sym, __VA_ARGS__}
#define GRAD_WORDS "the fused attention backward", "the fused attention backward", "fused attention backward pass"
#define ADD_WORDS "the additive attention score", "the additive attention pass", "additive attention pass"
#define V2_WORDS "the gatv2 attention score", "the gatv2 attention pass", "gatv2 attention pass"
#define QKV_WORDS(with) "the transformer attention score" with, "the transformer attention pass" with, "transformer attention pass"
#define COEF_WORDS "the export of the attention coefficients", "the attention-coefficient export", "attention-coefficient export"
#define FINISH(score) "Error, the " score " forward finish belongs to the block's last window!"
const AttnEntry kAttnEntries[] = {
    HNH_ATTN_ENTRY(GRAD, 1, PLAIN, hnh_attn_grad_row_csr_p, GRAD_WORDS, nullptr, w_head),
    HNH_ATTN_ENTRY(GRAD, 2, PLAIN, hnh_attn_grad_col_csr_p, GRAD_WORDS, nullptr, w_pair),
    HNH_ATTN_ENTRY(ADDITIVE, 0, PLAIN, hnh_attn_add_fwd_csr_p, ADD_WORDS, FINISH("additive"), w_scored),
    HNH_ATTN_ENTRY(ADDITIVE, 1, PLAIN, hnh_attn_add_row_csr_p, ADD_WORDS, nullptr, w_scored),
    HNH_ATTN_ENTRY(ADDITIVE, 2, PLAIN, hnh_attn_add_col_csr_p, ADD_WORDS, nullptr, w_add_packed),
    HNH_ATTN_ENTRY(ADDITIVE, 0, DROP, hnh_attn_drop_fwd_csr_p, ADD_WORDS, FINISH("additive"), w_add_packed),
    HNH_ATTN_ENTRY(ADDITIVE, 1, DROP, hnh_attn_drop_row_csr_p, ADD_WORDS, nullptr, w_add_packed),
    HNH_ATTN_ENTRY(ADDITIVE, 2, DROP, hnh_attn_drop_col_csr_p, ADD_WORDS, nullptr, w_add_packed),
    HNH_ATTN_ENTRY(GATV2, 0, PLAIN, hnh_attn_v2_fwd_csr_p, V2_WORDS, FINISH("gatv2"), w_head),
    HNH_ATTN_ENTRY(GATV2, 1, PLAIN, hnh_attn_v2_row_csr_p, V2_WORDS, nullptr, w_head),
    HNH_ATTN_ENTRY(GATV2, 2, PLAIN, hnh_attn_v2_col_csr_p, V2_WORDS, nullptr, w_packed),
    HNH_ATTN_ENTRY(QKV, 0, PLAIN, hnh_attn_qkv_fwd_csr_p, QKV_WORDS(""), FINISH("transformer"), w_kv),
    HNH_ATTN_ENTRY(QKV, 1, PLAIN, hnh_attn_qkv_row_csr_p, QKV_WORDS(""), nullptr, w_kv),
    HNH_ATTN_ENTRY(QKV, 2, PLAIN, hnh_attn_qkv_col_csr_p, QKV_WORDS(""), nullptr, w_packed),
    HNH_ATTN_ENTRY(QKV, 0, BIAS, hnh_attn_qkv_bias_fwd_csr_p, QKV_WORDS(" with an edge bias"), FINISH("transformer"), w_kv),
    HNH_ATTN_ENTRY(QKV, 1, BIAS, hnh_attn_qkv_bias_row_csr_p, QKV_WORDS(" with an edge bias"), nullptr, w_kv),
    HNH_ATTN_ENTRY(QKV, 2, BIAS, hnh_attn_qkv_bias_col_csr_p, QKV_WORDS(" with an edge bias"), nullptr, w_packed),
    HNH_ATTN_ENTRY(QKV, 1, BIAS_GRAD, hnh_attn_qkv_bias_grad_row_csr_p, QKV_WORDS(" with a learned edge bias"), nullptr, w_kv),
    HNH_ATTN_ENTRY(QKV, 2, BIAS_GRAD, hnh_attn_qkv_bias_grad_col_csr_p, QKV_WORDS(" with a learned edge bias"), nullptr, w_packed),
    HNH_ATTN_ENTRY(COEF, 0, PLAIN, hnh_attn_coef_csr_p, COEF_WORDS, nullptr, w_coef),
};
#undef HNH_ATTN_ENTRY
#undef GRAD_WORDS
#undef ADD_WORDS
#undef V2_WORDS
#undef QKV_WORDS
#undef COEF_WORDS
#undef FINISH
// attn_block calls a row through the signature of ONE member per variant: the members that share a call must share their type
template <typename F, typename... G>
constexpr bool kSameSignature = (std::is_same_v<F, G> && ...);
static_assert(kSameSignature<decltype(&::hnh_attn_grad_row_csr_p), decltype(&::hnh_attn_grad_col_csr_p)>);
static_assert(kSameSignature<decltype(&::hnh_attn_add_fwd_csr_p), decltype(&::hnh_attn_add_row_csr_p), decltype(&::hnh_attn_add_col_csr_p)>);
static_assert(kSameSignature<decltype(&::hnh_attn_drop_fwd_csr_p), decltype(&::hnh_attn_drop_row_csr_p), decltype(&::hnh_attn_drop_col_csr_p)>);
static_assert(kSameSignature<decltype(&::hnh_attn_v2_fwd_csr_p), decltype(&::hnh_attn_v2_row_csr_p), decltype(&::hnh_attn_v2_col_csr_p)>);
static_assert(kSameSignature<decltype(&::hnh_attn_qkv_fwd_csr_p), decltype(&::hnh_attn_qkv_row_csr_p), decltype(&::hnh_attn_qkv_col_csr_p)>);
static_assert(kSameSignature<decltype(&::hnh_attn_qkv_bias_fwd_csr_p), decltype(&::hnh_attn_qkv_bias_row_csr_p), decltype(&::hnh_attn_qkv_bias_col_csr_p)>);
static_assert(kSameSignature<decltype(&::hnh_attn_qkv_bias_grad_row_csr_p), decltype(&::hnh_attn_qkv_bias_grad_col_csr_p)>);
const AttnEntry& attn_entry(const AttnPass& p) {
    if (p.dbias != nullptr && p.pass == 0) hnh::fatal("Error, the edge bias's gradient belongs to the backward passes!");
    for (const AttnEntry& e : kAttnEntries)
        if (e.family == p.family() && e.pass == p.pass && e.variant == variant_of(p)) return e;
    hnh::fatal("Error, attn_local: the family has no pass " + std::to_string(p.pass) + "!");
    return kAttnEntries[0];
}
}  // namespace

std::string KernelImplementation::attn_missing(const AttnPass& pass) {
    return std::string("Error, the kernel implementation has no ") + attn_entry(pass).noun + " (KernelImplementation::attn_local)!";
}

bool KernelImplementation::attn_local(SpmatLocal& S, int block, const AttnPass& pass, unsigned flags, int64_t rows, bool finish) {
    StandardKernel* k = dynamic_cast<StandardKernel*>(this);
    return k != nullptr && k->attn_block(S, block, pass, flags, rows, finish);
}

// Every attention pass, next to fused_local: the entry point and its words from the table, the shared block and window handling, and the
// one place where the families differ, their entry points' signatures.
bool StandardKernel::attn_block(SpmatLocal& S, int block, const AttnPass& pass, unsigned flags, int64_t rows, bool finish) {
    hnh::World* w = S.world;
    const AttnEntry& e = attn_entry(pass);
    void* fn = e.fn(*w->be);
    if (fn == nullptr) throw hnh::Error(w->be->missing_kernel(e.feature, e.symbol));
    const bool closes = pass.forward() && finish;
    const unsigned f = flags | (closes ? HNH_ATTN_FINISH : 0u);
    CSRLocal* blk = S.csr_blocks[block];  // (its lent slices: see attn_local)
    attn_block_call(S, block, rows, e.label, closes ? e.finish_text : nullptr, e.width(pass), [&](const hnh_csr_block& d, const hnh_csr_window* win) {
        hnh_ctx* c = w->ctx;
        const int s = HNH_STREAM_COMPUTE;
        auto as = [fn](auto* member) { return reinterpret_cast<decltype(member)>(fn); };  // fn with a Backend member's signature, which a variant's passes share
        const int rc = std::visit(
            [&](const auto& a) -> int {
                using Args = std::decay_t<decltype(a)>;
                if constexpr (std::is_same_v<Args, hnh_attn_grad>) return as(&::hnh_attn_grad_row_csr_p)(c, &d, &a, f, win, s);
                else if constexpr (std::is_same_v<Args, hnh_attn_add>)
                    return e.variant == DROP ? as(&::hnh_attn_drop_fwd_csr_p)(c, &d, &a, pass.drop, f, win, s) : as(&::hnh_attn_add_fwd_csr_p)(c, &d, &a, f, win, s);
                else if constexpr (std::is_same_v<Args, hnh_attn_v2>) return as(&::hnh_attn_v2_fwd_csr_p)(c, &d, &a, f, win, s);
                else if constexpr (std::is_same_v<Args, hnh_attn_qkv>) {
                    const double* bias = (blk && e.variant != PLAIN) ? blk->spmm_values : nullptr;
                    double* dbias = (blk && e.variant == BIAS_GRAD) ? blk->sddmm_dst : nullptr;
                    return e.variant == BIAS_GRAD ? as(&::hnh_attn_qkv_bias_grad_row_csr_p)(c, &d, &a, bias, dbias, pass.accumulate ? 1 : 0, f, win, s)
                           : e.variant == BIAS    ? as(&::hnh_attn_qkv_bias_fwd_csr_p)(c, &d, &a, bias, f, win, s)
                                                  : as(&::hnh_attn_qkv_fwd_csr_p)(c, &d, &a, f, win, s);
                } else {  // the coefficients go where an SDDMM's values would: the lent slice, or the block's own array
                    double* coef = blk == nullptr ? nullptr : (blk->sddmm_dst ? blk->sddmm_dst : blk->getActive()->values);
                    return as(&::hnh_attn_coef_csr_p)(c, &d, coef, &a, pass.drop, f, win, s);
                }
            },
            pass.args);
        w->check(rc, e.symbol);
    });
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
