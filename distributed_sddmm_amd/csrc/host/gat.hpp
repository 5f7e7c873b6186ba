// Multi-head graph attention forward pass — same classes as the reference's gat.hpp (GATLayer :25-41, GAT :50-113).
// Per head (computeSelfAttentionHead, gat.hpp:83-104):
//     A = buffers[i] * W_j            dense GEMM          -> hnh_gemm_f64 (fp64 MFMA: the path's one dense contraction)
//     B = A;  de_shift(&B, nullptr, k_spmmA)
//     e = SDDMM(A, B)  (S = 1)        algorithm(k_sddmmA, replicate)
//     e = LeakyReLU(e)                hnh_leaky_relu_f64 on the value vector
//     A = 0;  A = SpMM(e, B)          algorithm(k_spmmA, no re-replication: FusedMM by replication reuse)
//     buffers[i+1][:, j*w : (j+1)*w] = ReLU(A)            -> hnh_relu_store_cols_f64
// The reference leaves the weights zero and `leaky_relu_alpha` uninitialised (gat.hpp:55,78):
// it is a timing skeleton.  Here alpha defaults to 0.2 and weights are settable; like the reference, the product
// X * W uses each rank's LOCAL column slice of X (gat.hpp:88), so results are only meaningful for schedules that
// do not split R (1.5D dense shift), which is what the parity tests use.
//
// Backward pass (an addition: the reference's gat.hpp:43-48 leaves it as work in progress).  backwardPass(G), G = dL/d(last
// output), per head h of layer i from the last layer down, with X = buffers[i], out = buffers[i+1], f = features_per_head:
//     A = X * W_h, e = SDDMM(A, A)                 recomputed (the fused c = 1 forward never materialises e)
//     dZ = G[:, h f ..] * [out[:, h f ..] > 0]     hnh_relu_grad_cols_f64
//     da_ij = <dZ_i, A_j>;  a = LReLU(e), de = da * LReLU'(e)      in S layout and again in ST layout (hnh_leaky_relu_grad_f64)
//     dA = spmmA(de; A) + spmmB(a^T; dZ) + spmmB(de^T; A)         row side + the two column sides
// 4 SDDMM and 3 SpMM passes per head through the operator's own calls (S^T lives on other ranks: recomputing in ST layout is the
// communication-free way to the column sides).  Per layer, with dA_all = [dA_1 .. dA_H] (rows x H f):
//     dW_all = X^T * dA_all          ONE split-K GEMM (hnh_gemm_tn_f64), summed over the world: every global row lives on one rank
//     dX = dA_all * [W_1^T; ..; W_H^T]   hnh_gemm_f64: the G of layer i - 1, or the input gradient for layer 0
// Everything runs on the compute stream.  Supported where the forward pass is oracle.gat_forward's math and R is not split:
// 15d_fusion1 (any c) and 15d_fusion2 with c = 1.  The dense kernels are the optional group of include/hnh_grad.h.
//
// Attention mode (an addition): HNH_GAT_ATTENTION_NONE (the default) uses the LeakyReLU scores raw, as above;
// HNH_GAT_ATTENTION_SOFTMAX normalises them over each row's neighbourhood (Velickovic et al.):
//     s_ij = LeakyReLU(<A_i, A_j>),  lse_i = log sum_j exp(s_ij),  a_ij = exp(s_ij - lse_i),  out[:, h f ..] = ReLU(sum_j a_ij A_j)
// in ONE fused pass per head with an online softmax (include/hnh_attention.h; lse kept per (layer, head)).  Its backward pass is the
// one above with a in place of LeakyReLU(e) and, with delta_i = <dZ_i, out_i> and the lse and delta broadcast onto the nonzeros by
// width-1 SDDMMs in both layouts, de_ij = a_ij (da_ij - delta_i) LeakyReLU'(e_ij) (hnh_softmax_gate_f64).  15d_fusion2 with c = 1
// only: on every other schedule a row's nonzeros are summed across ranks, which a softmax cannot be.
//
// Backward mode (an addition): HNH_GAT_BACKWARD_UNFUSED (the default) is the pass above, seven operator calls per head.
// HNH_GAT_BACKWARD_FUSED computes the same dA = dArow + T1 + T2 in TWO passes per head (include/hnh_attn_grad.h):
//     row pass over S       A_i, dZ_i, lse_i, delta_i in registers, one gather of A_j: e, da, the gate and dA_i += de_ij A_j
//     column pass over S^T  A_j in registers, one gather of the packed P_i = [A_i | dZ_i | lse_i delta_i]: e, da, the gate with the
//                           gathered row's scalars, and dA_j += a_ij dZ_i + de_ij A_i
// straight into the head's column block of dA_all: no value vectors, no gate launches, no width-1 SDDMMs, no sum3.  15d_fusion2 with
// c = 1 only (the condition of the fused forward: a rank's own launches see all of a row's nonzeros and no output row is summed
// across ranks), heads of at most HNH_ATTN_GRAD_MAX_F features.  Switching the mode needs no new forward pass.
//
// Score (an addition): HNH_GAT_SCORE_DOT (the default) is everything above, e_ij = LeakyReLU(<A_i, A_j>).  HNH_GAT_SCORE_ADDITIVE scores an
// edge with the layer's two learned vectors (Velickovic et al.; head h uses the slices [h f, (h + 1) f) of GATLayer::a1 / a2):
//     s_i = <A_i, a1_h>,  t_j = <A_j, a2_h>,  z_ij = s_i + t_j,  e_ij = LeakyReLU(z_ij),  then the neighbourhood softmax as above.
// Forward: the product stage of a head also builds the scored operand M = [A (0) | s t] (one read of A), and the attention pass gathers
// ONE row of M per nonzero (include/hnh_attn_additive.h).  Backward, with dZ and delta as above:
//     dz_ij = a_ij (<dZ_i, A_j> - delta_i) LeakyReLU'(z_ij),  ds_i = sum_j dz_ij  (row pass over S),
//     dt_j = sum_i dz_ij,  dAgg_j = sum_i a_ij dZ_i  (column pass over S^T, gathering the packed Q_i = [dZ_i (0) | s_i lse_i delta_i 0]),
//     dA = dAgg + ds a1_h^T + dt a2_h^T,  da1_h = A^T ds,  da2_h = A^T dt  (attn_grads, summed over the world like dW).
// Supported where the softmax is (15d_fusion2 with c = 1, attention softmax) with heads of at most HNH_ATTN_ADD_MAX_F features; everything
// else raises before anything is launched.  With score ADDITIVE there is ONE backward implementation: set_backward is not consulted.
//
// HNH_GAT_SCORE_GATV2 (an addition; include/hnh_attn_v2.h) is Brody, Alon and Yahav's dynamic attention with shared weights: ONE learned vector
// per head (the slice [h f, (h + 1) f) of GATLayer::a1; a2 is kept and not used), the nonlinearity inside the contraction and none outside:
//     u_ijc = A_ic + A_jc,  sg_ijc = u_ijc > 0 ? 1 : alpha,  z_ij = sum_c a_c sg_ijc u_ijc,  then the neighbourhood softmax as above.
// Forward: one pass on the plain product A through the two-stream head pipeline of score DOT (no scored operand).  Backward, with dZ and delta
// as above and g_ij = p_ij (<dZ_i, A_j> - delta_i):
//     R_ic = sum_j g_ij sg_ijc  (row pass over S),  C_jc = sum_i g_ij sg_ijc,  dAgg_j = sum_i p_ij dZ_i  (column pass over S^T, gathering the
//     packed P_i = [A_i | dZ_i | lse_i delta_i] of the fused backward),  T = R + C,  dA = dAgg + T o a,  da_c = sum_r A_rc T_rc
// (LReLU(u) = sg (A_ic + A_jc), so sum_ij g sg u splits into the two sides: the gradient of a is one dense column sum, in the finishing pass).
// attn_grads keeps its (H f) x 2 shape: column 0 = da, column 1 = zeros.  Supported where score ADDITIVE is, without attention dropout; one
// backward implementation.
//
// HNH_GAT_SCORE_TRANSFORMER (an addition; include/hnh_attn_qkv.h) is scaled dot-product attention with separate projections (TransformerConv /
// UniMP, the graph transformers): per (layer, head) W_q and W_k (input_features x f, zero until set) next to the head's weight, which is W_v:
//     Q = X W_q,  K = X W_k,  V = X W_v,  s_ij = <Q_i, K_j> / sqrt(f)  (no LeakyReLU),  then the neighbourhood softmax as above over V.
// Forward: the head's product stage gives V; the attention stage on the compute stream makes Q and K (two more hnh_gemm_f64), packs
// [K | V] with hnh_attn_grad_pack_f64 (no scalars) and runs one pass that gathers a packed row per nonzero; the schedule runs at the packed
// width.  Backward, with dZ and delta as above and g_ij = p_ij (<dZ_i, V_j> - delta_i) / sqrt(f):
//     dQ_i = sum_j g_ij K_j  (row pass over S, gathering [K | V]),  dK_j = sum_i g_ij Q_i,  dV_j = sum_i p_ij dZ_i  (column pass over S^T,
//     gathering the packed [Q | dZ | lse delta]),  dW_v = X^T dV (weight_grads),  dW_q = X^T dQ,  dW_k = X^T dK (qk_weight_grads, summed over
//     the world like dW),  dX = dV W_v^T + dQ W_q^T + dK W_k^T in this order.
// W_q = W_k = 0 is a stationary point of both (uniform attention, dQ = dK = 0): callers initialise them.  Supported where score GATV2 is,
// without attention dropout; one backward implementation; attention_coefficients refuses this score.
//
// Dropout (an addition; set_dropout(attention_p, feature_p, seed), both rates 0 by default, which launches exactly the kernels above at
// their widths).  The masks are never stored: every pass recomputes them from Philox-4x32-10 keyed by (seed, layer, head, global row,
// global column) (include/hnh_attn_dropout.h), so they do not depend on the rank count, windows, panels or hub-row segments, and the
// backward column pass over S^T on another rank sees the forward pass's mask.  A change of rates or seed invalidates the stored
// forward pass, so backwardPass always differentiates the masks of the forward pass it belongs to.
//     attention_p > 0 (score ADDITIVE only): o_i = sum_j c m_ij a_ij A_j with c = 1 / (1 - p); lse and a_ij are those of ALL edges;
//         dz_ij = a_ij (c m_ij <dZ_i, A_j> - delta_i) LeakyReLU'(z_ij), dAgg_j = sum_i c m_ij a_ij dZ_i.  The gathered row's global id
//         travels in the operand: the head pipeline builds M' = [A (0) | s t | id 0] (fp + 4 columns) and the backward Q' = [dZ (0) | s
//         lse delta id], and the schedule runs at that width.
//     feature_p > 0 (wherever the passes themselves are supported, one dense block per rank): layer l keeps Xd = c_q mask o X, made on
//         the compute stream before the product stage starts; Xd replaces X in the head products and in dW = Xd^T dA_all, and
//         input_grads[l] = c_q mask o (dA_all Wt).
//
// Training (an addition; include/hnh_train.h).  set_labels keeps this rank's slice of the labels on the device (local row r is global row
// aSubmatrices[0].topRow + r, the numbering of the output's rows; a negative label or a row outside the mask is not in the loss) and sums the
// labelled count over the world once.  loss() is ONE pass over the last buffer: masked softmax cross-entropy of z = the mean over the last
// layer's heads (HNH_GAT_HEADS_MEAN) or of the whole row (HNH_GAT_HEADS_CONCAT), with loss_sum, correct and G = dL/d(output) from the same
// read; the two sums are all-reduced like dW.  optimizer_step() is one table-driven launch over every W (and a1, a2 with score ADDITIVE):
// weight_grads / attn_grads are identical on every rank, so every rank applies the same update and the parameters stay equal bit for bit
// without a broadcast.  train_step() = [seed + 1 when a dropout rate is nonzero] forwardPass, loss into an internal G, backwardPass,
// optimizer_step, all on the compute stream; the host waits once, for the two scalars (of the parameters BEFORE the update).
//
// The multi-label head (an addition; include/hnh_train_multilabel.h).  set_multilabel_targets keeps this rank's rows of the M x classes
// 0/1 targets bit-packed on the device with its rows of the mask and the class weights, and sums the selected row count over the world once.
// Until the next set_labels, loss / train_step / evaluate then run ONE pass of hnh_bce_rows_f64 in place of hnh_xent_rows_f64: the weighted
// sigmoid cross-entropy of z (heads as above), mean over selected rows x classes, with tp / fp / fn of the prediction z > 0 and G from the
// same read; the four sums are all-reduced, the pair's second value is micro-F1 = 2 tp / (2 tp + fp + fn), and multilabel_counts() hands out
// the counts.  No row is staged, so HNH_XENT_MAX_WIDTH does not apply.  A model that never calls it launches what it launched before.
//
// Gradient clipping, AdamW and learning-rate schedules (an addition; include/hnh_train_clip.h; set_grad_clip, optimizer kind
// HNH_OPTIM_ADAMW, set_learning_rate, set_lr_schedule; all off by default, which launches exactly the kernels above).  With clipping on,
// optimizer_step first runs hnh_grad_sumsq_f64 over learned_parameters(): the replicated tensors into one sum without a collective (their
// gradients are bit-equal on every rank), the S-order copy of every learned edge bias into a second one that is summed over the world;
// the update then goes through hnh_optim_step_clip_f64, where every thread derives coef = min(1, max_norm / (norm + 1e-6)) from the two
// sums in device memory.  No host synchronisation is added: train_step still waits once, and grad_norm() reads the sums lazily.  The
// schedule is host arithmetic on the step's lr.
//
// Output activation (an addition; set_activation(layer, mode), HNH_GAT_ACT_RELU on every layer by default, which launches exactly the kernels
// above).  out[:, h f ..] = phi_l(o) with phi in {relu, elu, identity} leaves the finishing launch of the softmax and additive forward passes
// (the HNH_ATTN_ACT_* flags of include/hnh_attention.h).  The backward pass keeps no pre-activation: for a non-ReLU layer ONE pass
// (hnh_act_grad_cols_f64, include/hnh_grad.h) makes dZ and delta of a head from G and the stored output, in place of hnh_relu_grad_cols_f64 and
// hnh_rowdot_cols_f64:  identity  dZ = G, delta_i = <G_i, out_i>;  elu  dZ = G where out >= 0 and G (1 + out) below, delta_i = sum_c dZ_ic o_ic
// with o = log1p(out) below 0 (the term is 0 where 1 + out == 0).  Supported with attention softmax (score dot or additive, any dropout rates)
// on 15d_fusion2 with c = 1; attention none keeps ReLU only, and everything else raises before anything is launched.
// The published network is activation elu on the hidden layers and identity on the last with HNH_GAT_HEADS_MEAN: the loss then averages the raw
// head aggregates.  With the default relu on the last layer the heads pass through the ReLU epilogue before they are averaged.
//
// Bias and skip connections (an addition; include/hnh_gat_skip.h; set_bias(layer, b), set_residual(layer, mode), both off by default, which
// launches exactly the kernels above).  out[:, h f ..] = phi_l(o_h + r[:, h f ..] + b[h f ..]) with r = 0 (HNH_GAT_RESIDUAL_NONE), the layer
// input X (IDENTITY, needs input_features == H f) or X W_res (PROJECTION, W_res learned, kept per head as input_features x f operands of
// hnh_gemm_f64); X is Xd under feature dropout, what the head products use.  Forward: the addend r + b of head h belongs to the head's
// product stage (the auxiliary stream, next to head_product and head_scores): for PROJECTION one more product X W_res_h into a scratch,
// then hnh_skip_addend_cols_f64 writes the addend into the head's column block of buffers[l + 1], where the head's finishing launch on
// the compute stream reads it and overwrites it with the activated sum (HNH_ATTN_ADDEND next to activation_flag).  Order: ev_gemm of the
// head's stage orders the addend before the finish; the two streams write disjoint column blocks; and every earlier reader of
// buffers[l + 1] (the next layer's feature mask, the loss, the backward pass, the coefficient export, copies to the host) runs on the
// compute stream before the layer's ev_input mark, which the auxiliary stream awaits before its first write, or on the auxiliary stream
// itself (the next layer's products of the previous pass), which is in order.  Backward: hnh_skip_grad_cols_f64 in place of
// hnh_relu_grad_cols_f64 / hnh_act_grad_cols_f64, with res = X's column block (IDENTITY) or the recomputed X W_res_h (PROJECTION): the same dZ,
// delta_i = <dZ_i, phi^{-1}(out_i) - r_i - b> (head_delta hands it out, ReLU included), and every head's dZ also into dZ_all (rows x H f).
// After the head loop, on the compute stream: bias_grads[l] = colsum(dZ_all) (hnh_colsum_f64) and res_weight_grads[l] = X^T dZ_all
// (hnh_gemm_tn_f64), both summed over the world like dW, and dX += dZ_all W_res^T (PROJECTION) or dZ_all (IDENTITY) before the feature
// mask.  Neither a pre-activation nor an addend is kept between the passes.  Supported with attention softmax (every score, both backward
// modes, any dropout the score allows, any activation) on 15d_fusion2 with c = 1; everything else raises before anything is launched
// (check_skip_supported).  optimizer_step appends every enabled bias and W_res to its table; weight decay applies to them as to W.
//
// Layer normalisation (an addition; include/hnh_gat_norm.h; set_norm(layer, mode, eps), set_norm_weights(layer, gamma, beta), off on every
// layer by default, which launches exactly the kernels above).  out = phi_l(gamma o xh + beta) with xh the WHOLE row z = o + r + b (all heads
// side by side, C = H f columns) normalised: mu = mean_c z, var = mean_c (z - mu)^2 (biased, two-pass), xh = (z - mu) / sqrt(var + eps); gamma = 1
// and beta = 0 until set, both learned.  Forward: a normalised layer l keeps pre_[l] (rows x H f: ONE MORE MATRIX OF THE LAYER OUTPUT'S SIZE, the
// feature's memory cost) and norm_stats_[l] (rows x 2: mu, 1 / sigma).  The heads' addend (head_addend) and the finishing launch of every
// score's forward pass target pre_[l] with the identity activation flag where they target buffers[l + 1] otherwise (head_target / head_act), and
// after the layer's last head one hnh_layernorm_fwd_f64 on the compute stream writes buffers[l + 1], which everything downstream reads as
// before (the next layer, the loss, evaluate, the coefficient export, copies to the host).  Order: the argument of the addend above carries
// over to pre_[l] word for word: ev_gemm of the head's stage orders the addend before the finish; the two streams write disjoint column blocks;
// and every earlier reader of pre_[l] (the previous pass's normalisation and backward pass) runs on the compute stream before the layer's
// ev_input mark, which the auxiliary stream awaits before its first write; pre_[l] is allocated before that mark, like the product buffers.
// Backward: backward_layer(i, G) first runs hnh_layernorm_bwd_f64 from G, pre_[i] and the stats into a scratch G' (dz of the formulas in the
// header; y is recomputed), sums norm_grads_[i] = [dgamma; dbeta] over the world as db is summed, and then runs the layer code above with G' in
// G's place, pre_[i] in the stored output's place and the identity in the activation's place: head_dz / hnh_skip_grad_cols_f64 /
// hnh_act_grad_cols_f64 do for it what they do for an identity layer, and nothing in the scores' backward passes changes.  Supported where the
// activations are (attention softmax, every score, both backward modes, any dropout the score allows, bias and both residuals) on 15d_fusion2
// with c = 1 and rows of at most HNH_NORM_MAX_COLS values; everything else raises before anything is launched, naming the layer
// (check_norm_supported).  optimizer_step appends gamma and beta of every normalised layer behind the layer's other entries; like the edge
// bias they are NEVER decayed (decay would pull gamma to 0).  dgamma and dbeta are identical on every rank, so the two stay equal bit for bit.
#pragma once
#include "dense_shift_15d.hpp"
#include "distributed_sparse.hpp"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include "hnh_dist.h"
// HNH_GAT_KERNEL(name): an entry of require_kernels' list.  HNH_GAT_CALL(name, arguments after the context): one kernel call on the
// operator's world, refused with the kernel's name.
#define HNH_GAT_KERNEL(name) {(const void*)d_ops->world->be->name, #name}
#define HNH_GAT_CALL(name, ...) d_ops->world->check(d_ops->world->be->name(d_ops->world->ctx, __VA_ARGS__), #name)

class GATLayer {
public:
    int input_features, features_per_head, num_heads;
    std::vector<DenseMatrix> wMats;
    VectorXd a1, a2;
    GATLayer(int input_features, int features_per_head, int num_heads)
        : input_features(input_features), features_per_head(features_per_head), num_heads(num_heads) {}
};

class GAT {
public:
    Distributed_Sparse* d_ops;
    std::vector<GATLayer> layers;
    std::vector<DenseMatrix> buffers;
    double leaky_relu_alpha = 0.2;

    GAT(std::vector<GATLayer>& l_input, Distributed_Sparse* d_ops) {
        if (l_input.empty()) hnh::fatal("Error, a GAT needs at least one layer!");
        this->d_ops = d_ops;
        world_ = d_ops->world;  // not owned by the operator: benchmark_dist.cpp:166 deletes d_ops while its GAT is still alive
        layers = l_input;
        act_.assign(layers.size(), HNH_GAT_ACT_RELU);
        res_mode_.assign(layers.size(), HNH_GAT_RESIDUAL_NONE);
        norm_.assign(layers.size(), HNH_GAT_NORM_NONE);
        norm_eps_.assign(layers.size(), 1e-5);
        for (auto* v : {&norm_gain_, &norm_shift_, &norm_grads_, &pre_, &norm_stats_}) v->assign(layers.size(), DenseMatrix());
        norm_grads_held_.assign(layers.size(), 0);
        bias_on_.assign(layers.size(), 0);
        bias_.assign(layers.size(), DenseMatrix());
        edge_bias_on_.assign(layers.size(), 0);
        for (auto& e : edge_bias_) e.assign(layers.size(), VectorXd());
        edge_bias_learned_.assign(layers.size(), 0);
        dbias_held_.assign(layers.size(), 0);
        for (auto& e : dbias_) e.assign(layers.size(), VectorXd());
        w_res_.assign(layers.size(), std::vector<DenseMatrix>());
        for (auto& w : w_qk_) w.assign(layers.size(), std::vector<DenseMatrix>());
        d_ops->setRValue(layers[0].input_features);
        buffers.push_back(d_ops->like_B_matrix(0.0));
        for (size_t i = 0; i < layers.size(); i++) {
            if (i > 0 && layers[i].input_features != layers[i - 1].num_heads * layers[i - 1].features_per_head)
                hnh::fatal("Error, GAT layer input width does not match the previous layer's output width!");
            d_ops->setRValue(layers[i].features_per_head * layers[i].num_heads);
            buffers.push_back(d_ops->like_A_matrix(0.0));
            d_ops->setRValue(layers[i].features_per_head);
            for (int j = 0; j < layers[i].num_heads; j++)
                layers[i].wMats.push_back(DenseMatrix::Constant(buffers[i].cols(), d_ops->localAcols, 0.0));
        }
    }

    ~GAT() {  // never touches d_ops: the reference's harness has deleted it by now (benchmark_dist.cpp:166 vs the unique_ptr's scope)
        hnh::World* w = world_;
        if (w == nullptr) return;
        w->sync_all_nothrow();  // the events below may still be waited on
        for (void* e : {ev_input, ev_gemm[0], ev_gemm[1], ev_head[0], ev_head[1]})
            if (e) w->event_destroy(e);
    }
    GAT(const GAT&) = delete;
    GAT& operator=(const GAT&) = delete;

    // HNH_GAT_ATTENTION_NONE | HNH_GAT_ATTENTION_SOFTMAX (include/hnh_dist.h); a change invalidates the stored forward pass
    int attention() const { return attention_; }
    void set_attention(int mode) {
        if (mode != HNH_GAT_ATTENTION_NONE && mode != HNH_GAT_ATTENTION_SOFTMAX)
            throw hnh::Error("Error, unknown GAT attention mode " + std::to_string(mode) + " (none = 0, softmax = 1)!");
        if (mode != attention_) invalidate_forward();
        attention_ = mode;
    }

    // HNH_GAT_SCORE_DOT | HNH_GAT_SCORE_ADDITIVE | HNH_GAT_SCORE_GATV2 | HNH_GAT_SCORE_TRANSFORMER (include/hnh_dist.h); a change invalidates
    // the stored forward pass, and one away from TRANSFORMER drops qk_weight_grads
    int score() const { return score_; }
    void set_score(int mode) {
        if (mode != HNH_GAT_SCORE_DOT && mode != HNH_GAT_SCORE_ADDITIVE && mode != HNH_GAT_SCORE_GATV2 && mode != HNH_GAT_SCORE_TRANSFORMER)
            throw hnh::Error("Error, unknown GAT score " + std::to_string(mode) + " (dot = 0, additive = 1, gatv2 = 2)!");
        if (mode != score_) {
            invalidate_forward();
            // (leaving score TRANSFORMER: no later backward pass refreshes dW_q and dW_k, so their getter refuses rather than hand out old ones)
            if (score_ == HNH_GAT_SCORE_TRANSFORMER) {
                for (auto& gq : qk_weight_grads) gq.clear();
                for (size_t l = 0; l < layers.size(); l++) drop_edge_bias_grad((int)l);
            }
        }
        score_ = mode;
    }

    // The transformer score's W_q (which = 0) and W_k (which = 1) of (layer i, head h): HOST matrices, row-major input_features x
    // features_per_head like the head's weight, zero until set, allocated on first use.  Setting one invalidates the stored forward pass.
    void set_qk_weight(int i, int h, int which, const double* host) {
        check_qk(i, h, which);
        if (host == nullptr) throw hnh::Error("Error, GAT set_qk_weight: null pointer!");
        ensure_qk_weights(i);
        w_qk_[which][(size_t)i][(size_t)h].copy_from_host(host);
        invalidate_forward();
    }
    void get_qk_weight(int i, int h, int which, double* host) {
        check_qk(i, h, which);
        if (host == nullptr) throw hnh::Error("Error, GAT get_qk_weight: null pointer!");
        ensure_qk_weights(i);
        w_qk_[which][(size_t)i][(size_t)h].copy_to_host(host);
    }

    // HNH_GAT_ACT_RELU | HNH_GAT_ACT_ELU | HNH_GAT_ACT_IDENTITY of layer i's output (include/hnh_dist.h); a change invalidates the stored
    // forward pass.  Kept here, not in GATLayer, whose size drivers compiled against the previous headers embed.
    int activation(int i) const {
        check_layer(i);
        return act_[(size_t)i];
    }
    void set_activation(int i, int mode) {
        check_layer(i);
        if (mode != HNH_GAT_ACT_RELU && mode != HNH_GAT_ACT_ELU && mode != HNH_GAT_ACT_IDENTITY)
            throw hnh::Error("Error, unknown GAT activation " + std::to_string(mode) + " (relu = 0, elu = 1, identity = 2)!");
        if (mode != act_[(size_t)i]) invalidate_forward();
        act_[(size_t)i] = mode;
    }

    // Skip connection of layer i (include/hnh_dist.h): HNH_GAT_RESIDUAL_NONE | _IDENTITY | _PROJECTION; a change invalidates the stored forward
    // pass.  PROJECTION allocates W_res (zero until set) on first use.  Kept here, not in GATLayer, for set_activation's reason.
    int residual(int i) const {
        check_layer(i);
        return res_mode_[(size_t)i];
    }
    void set_residual(int i, int mode) {
        check_layer(i);
        if (mode != HNH_GAT_RESIDUAL_NONE && mode != HNH_GAT_RESIDUAL_IDENTITY && mode != HNH_GAT_RESIDUAL_PROJECTION)
            throw hnh::Error("Error, unknown GAT residual mode " + std::to_string(mode) + " (none = 0, identity = 1, projection = 2)!");
        const GATLayer& L = layers[(size_t)i];
        if (mode == HNH_GAT_RESIDUAL_IDENTITY && L.input_features != L.num_heads * L.features_per_head)
            throw hnh::Error("Error, GAT residual identity of layer " + std::to_string(i) + " needs input_features == num_heads * features_per_head, not " +
                             std::to_string(L.input_features) + " and " + std::to_string(L.num_heads * L.features_per_head) + ": use residual projection!");
        if (mode == HNH_GAT_RESIDUAL_PROJECTION) ensure_residual_weight(i);
        if (mode != res_mode_[(size_t)i]) invalidate_forward();
        res_mode_[(size_t)i] = mode;
    }
    // W_res of layer i as one HOST matrix, row-major input_features x (num_heads * features_per_head); the device keeps it per head
    void set_residual_weight(int i, const double* host) {
        check_layer(i);
        if (host == nullptr) throw hnh::Error("Error, GAT set_residual_weight: null pointer!");
        ensure_residual_weight(i);
        copy_residual_weight(i, host, nullptr);
        invalidate_forward();
    }
    void get_residual_weight(int i, double* host) {
        check_layer(i);
        if (host == nullptr) throw hnh::Error("Error, GAT get_residual_weight: null pointer!");
        if (w_res_[(size_t)i].empty()) throw hnh::Error("Error, GAT layer " + std::to_string(i) + " has no residual weight: set_residual(layer, projection) first!");
        copy_residual_weight(i, nullptr, host);
    }
    // The bias of layer i (num_heads * features_per_head HOST entries); nullptr switches it off.  Invalidates the stored forward pass.
    bool has_bias(int i) const {
        check_layer(i);
        return bias_on_[(size_t)i] != 0;
    }
    void set_bias(int i, const double* host) {
        check_layer(i);
        if (host == nullptr) {
            if (bias_on_[(size_t)i]) invalidate_forward();
            bias_on_[(size_t)i] = 0;
            return;
        }
        const GATLayer& L = layers[(size_t)i];
        const int64_t hf = (int64_t)L.num_heads * L.features_per_head;
        DenseMatrix& b = bias_[(size_t)i];
        if (b.rows() != hf || b.cols() != 1) b = DenseMatrix(hf, 1);
        b.copy_from_host(host);
        bias_on_[(size_t)i] = 1;
        invalidate_forward();
    }
    void get_bias(int i, double* host) {
        check_layer(i);
        if (host == nullptr) throw hnh::Error("Error, GAT get_bias: null pointer!");
        if (!bias_on_[(size_t)i]) throw hnh::Error("Error, GAT layer " + std::to_string(i) + " has no bias: set_bias first!");
        bias_[(size_t)i].copy_to_host(host);
    }

    // Layer normalisation of layer i (include/hnh_gat_norm.h): HNH_GAT_NORM_NONE | HNH_GAT_NORM_LAYER with its eps (> 0, finite; kept while
    // the norm is off).  gamma = 1 and beta = 0 until set_norm_weights.  A change invalidates the stored forward pass; a refused call leaves
    // the object as it was.  Kept here, not in GATLayer, for set_activation's reason.
    int norm(int i) const {
        check_layer(i);
        return norm_[(size_t)i];
    }
    double norm_eps(int i) const {
        check_layer(i);
        return norm_eps_[(size_t)i];
    }
    void set_norm(int i, int mode, double eps) {
        check_layer(i);
        if (mode != HNH_GAT_NORM_NONE && mode != HNH_GAT_NORM_LAYER)
            throw hnh::Error("Error, unknown GAT norm mode " + std::to_string(mode) + " (none = 0, layer = 1)!");
        if (!(eps > 0.0) || !std::isfinite(eps))
            throw hnh::Error("Error, GAT set_norm of layer " + std::to_string(i) + " needs a positive finite eps, not " + std::to_string(eps) + "!");
        if (mode == HNH_GAT_NORM_LAYER) ensure_norm_weights(i);
        if (mode != norm_[(size_t)i] || eps != norm_eps_[(size_t)i]) {
            invalidate_forward();
            norm_grads_held_[(size_t)i] = 0;
        }
        norm_[(size_t)i] = mode;
        norm_eps_[(size_t)i] = eps;
    }
    // gamma and beta of layer i: `n` = num_heads * features_per_head HOST entries each
    void set_norm_weights(int i, const double* gamma, const double* beta, int64_t n) {
        check_norm_vectors(i, gamma, beta, n, "set_norm_weights");
        ensure_norm_weights(i);
        norm_gain_[(size_t)i].copy_from_host(gamma);
        norm_shift_[(size_t)i].copy_from_host(beta);
        invalidate_forward();
    }
    void get_norm_weights(int i, double* gamma, double* beta, int64_t n) {
        check_norm_vectors(i, gamma, beta, n, "get_norm_weights");
        ensure_norm_weights(i);
        norm_gain_[(size_t)i].copy_to_host(gamma);
        norm_shift_[(size_t)i].copy_to_host(beta);
    }
    // dL/dgamma and dL/dbeta of layer i from the last backwardPass (the same on every rank); refuses before one with the layer normalised
    void get_norm_grad(int i, double* dgamma, double* dbeta, int64_t n) {
        check_norm_vectors(i, dgamma, dbeta, n, "get_norm_grad");
        const DenseMatrix& g = norm_grads_[(size_t)i];
        if (norm_[(size_t)i] != HNH_GAT_NORM_LAYER || !norm_grads_held_[(size_t)i] || g.rows() != 2 || g.cols() != n)
            throw hnh::Error("Error, no GAT norm gradient of layer " + std::to_string(i) + " yet: call backwardPass with set_norm(layer, layer) first!");
        hnh::World* w = d_ops->world;
        w->copy(dgamma, g.data(), sizeof(double) * (size_t)n, HNH_COPY_D2H, HNH_STREAM_COMPUTE);
        w->copy(dbeta, g.data() + n, sizeof(double) * (size_t)n, HNH_COPY_D2H, HNH_STREAM_COMPUTE);
        w->sync(HNH_STREAM_COMPUTE);
    }

    // The per-edge bias of layer i's logits (include/hnh_attn_edge.h; score TRANSFORMER only, checked by forwardPass): one finite value per
    // nonzero of S on this rank, shared by the layer's heads and not learned, given TWICE: `s` in the like_S_values layout (the forward and
    // the backward row pass) and `st` in the like_ST_values layout (the backward column pass over S^T).  The caller keeps the two in
    // agreement: entry e of S and the entry of S^T that is the same nonzero carry the same value (S_coordinates / ST_coordinates name
    // them; two copies of a repeated pair may differ).  Both are copied, device to device; both null clears the bias, and the layer then
    // launches what it launched before.  A very negative value (-1e300) removes an edge from every row that keeps an edge of moderate
    // bias; a row's largest bias should stay within +-1e6, and a row of several edges that are ALL switched off is not supported (the
    // backward pass cannot recover 1 / degree from an lse of -1e300: include/hnh_attn_edge.h); -inf is not supported.  A change
    // invalidates the stored forward pass; a refused call leaves the object as it was.
    bool has_edge_bias(int i) const {
        check_layer(i);
        return edge_bias_on_[(size_t)i] != 0;
    }
    void set_edge_bias(int i, const VectorXd* s, const VectorXd* st) {
        check_layer(i);
        if (s == nullptr && st == nullptr) {
            if (edge_bias_on_[(size_t)i]) invalidate_forward();
            edge_bias_on_[(size_t)i] = 0;
            for (auto& e : edge_bias_) e[(size_t)i] = VectorXd();
            edge_bias_learned_[(size_t)i] = 0;  // (no bias, nothing to learn: the switch goes with it)
            drop_edge_bias_grad(i);
            return;
        }
        if (s == nullptr || st == nullptr)
            throw hnh::Error(std::string("Error, GAT set_edge_bias needs the bias in both orders: the ") + (s == nullptr ? "like_S_values" : "like_ST_values") +
                             " vector is null (both null clears the bias)!");
        if (edge_len_[0] < 0) {  // (the schedule says its layouts' lengths through the vectors it makes: asked once per object)
            edge_len_[0] = d_ops->like_S_values(0.0).size();
            edge_len_[1] = d_ops->like_ST_values(0.0).size();
        }
        const int64_t want[2] = {edge_len_[0], edge_len_[1]};
        const VectorXd* in[2] = {s, st};
        for (int k = 0; k < 2; k++)
            if (in[k]->size() != want[k])
                throw hnh::Error(std::string("Error, GAT set_edge_bias needs a vector of ") + (k == 0 ? "like_S_values" : "like_ST_values") + " length: " +
                                 std::to_string(want[k]) + " entries, not " + std::to_string(in[k]->size()) + "!");
        hnh::World* w = d_ops->world;
        for (int k = 0; k < 2; k++) {
            VectorXd& mine = edge_bias_[k][(size_t)i];
            if (mine.size() != want[k]) mine = VectorXd(want[k]);
            if (want[k] > 0) w->copy(mine.data(), in[k]->data(), sizeof(double) * (size_t)want[k], HNH_COPY_D2D, HNH_STREAM_COMPUTE);
        }
        edge_bias_on_[(size_t)i] = 1;
        invalidate_forward();
    }

    // A LEARNED edge bias (include/hnh_attn_edge_grad.h): the layer's bias becomes a parameter.  backwardPass then also computes
    //     dL/db_e = sum_h p_e^h (<dZ_i^h, V_j^h> - delta_i^h)        (heads added in the order h = 0 .. H-1)
    // with the two backward passes' grad entry points (accumulate = (h > 0)): the row pass writes it in S's order, the column pass in
    // S^T's, and optimizer_step updates each copy of the bias from the gradient of its own pass (the two copies are both parameters, as
    // ALS keeps ground_truth and ground_truth_transpose; both passes compute the same expression from the same operands, so the copies
    // agree to rounding, and two entries that start equal and get equal gradients stay equal).  Every rank holds the bias of its own
    // nonzeros only: the gradient needs no all-reduce.  THE BIAS IS NEVER DECAYED: optimizer_step updates these tensors in a call of
    // their own with weight_decay = 0 (same step count, same hyper-parameters otherwise), so an entry at -1e300 (a switched-off edge),
    // whose p_e and hence gradient are exactly 0 in every head and whose moments therefore stay 0, stays -1e300 to the bit under Adam
    // (eps > 0) and SGD; decay would multiply it.  Refused by name unless the layer has an edge bias; clearing the bias clears the
    // switch.  The forward pass does not depend on the switch, so the stored pass stays valid; switching it off drops the gradient.
    bool edge_bias_learned(int i) const {
        check_layer(i);
        return edge_bias_learned_[(size_t)i] != 0;
    }
    void set_edge_bias_learned(int i, bool on) {
        check_layer(i);
        if (on && !edge_bias_on_[(size_t)i])
            throw hnh::Error("Error, GAT set_edge_bias_learned: layer " + std::to_string(i) + " has no edge bias to learn (set_edge_bias first)!");
        edge_bias_learned_[(size_t)i] = on ? 1 : 0;
        if (!on) drop_edge_bias_grad(i);
    }
    // The bias of layer i as it stands (which = 0: S's order, like_S_values; 1: S^T's order, like_ST_values), device to device into `out`
    void get_edge_bias(int i, int which, VectorXd& out) {
        check_edge_which(i, which);
        if (!edge_bias_on_[(size_t)i]) throw hnh::Error("Error, GAT get_edge_bias: layer " + std::to_string(i) + " has no edge bias!");
        copy_edge_vector(edge_bias_[which][(size_t)i], out, "get_edge_bias");
    }
    // dL/db of layer i from the last backwardPass, in the same two orders.  Refuses before a backward pass with the layer's bias learned,
    // and after whatever dropped it: the switch or the bias cleared, a score other than TRANSFORMER set.
    void edge_bias_grad(int i, int which, VectorXd& out) {
        check_edge_which(i, which);
        if (!edge_bias_learned_[(size_t)i] || !dbias_held_[(size_t)i])
            throw hnh::Error("Error, no GAT edge-bias gradient of layer " + std::to_string(i) +
                             " yet: call backwardPass with set_edge_bias_learned on this layer first!");
        copy_edge_vector(dbias_[which][(size_t)i], out, "edge_bias_grad");
    }

    // Dropout (include/hnh_attn_dropout.h): rates in [0, 1) on the attention coefficients (score ADDITIVE only; checked by forwardPass)
    // and on every layer's input, masks keyed by `seed`.  (0, 0) is the default: today's kernels at today's widths.  A change
    // invalidates the stored forward pass.
    double attention_dropout() const { return attn_p_; }
    double feature_dropout() const { return feat_p_; }
    uint64_t dropout_seed() const { return seed_; }
    void set_dropout(double attention_p, double feature_p, uint64_t seed) {
        for (double p : {attention_p, feature_p})
            if (!(p >= 0.0 && p < 1.0)) throw hnh::Error("Error, GAT dropout rates must lie in [0, 1), not " + std::to_string(p) + "!");
        attn_p_ = attention_p;
        feat_p_ = feature_p;
        seed_ = seed;
        invalidate_forward();
    }
    void set_dropout_seed(uint64_t seed) {
        seed_ = seed;
        invalidate_forward();
    }

    // The additive score's vectors of a layer (GATLayer::a1 / a2: num_heads * features_per_head entries each, zero until set; head h
    // uses the slice [h f, (h + 1) f)), allocated on first use.  Score GATV2 reads a1 alone.
    void ensure_attn_vectors(int i) {
        GATLayer& L = layers.at((size_t)i);
        const int64_t n = (int64_t)L.num_heads * L.features_per_head;
        if (L.a1.size() != n) L.a1 = VectorXd::Constant(n, 0.0);
        if (L.a2.size() != n) L.a2 = VectorXd::Constant(n, 0.0);
    }
    void set_attn_vectors(int i, int h, const double* a1_host, const double* a2_host) {
        ensure_attn_vectors(i);
        if (h < 0 || h >= layers[(size_t)i].num_heads) throw hnh::Error("Error, GAT head index out of range!");
        copy_attn_vectors(i, h, const_cast<double*>(a1_host), const_cast<double*>(a2_host), HNH_COPY_H2D);
        invalidate_forward();
    }

    // HNH_GAT_BACKWARD_UNFUSED | HNH_GAT_BACKWARD_FUSED (include/hnh_dist.h); the stored forward pass serves either
    // (not consulted with score ADDITIVE, which has one backward implementation)
    int backward() const { return backward_; }
    void set_backward(int mode) {
        if (mode != HNH_GAT_BACKWARD_UNFUSED && mode != HNH_GAT_BACKWARD_FUSED)
            throw hnh::Error("Error, unknown GAT backward mode " + std::to_string(mode) + " (unfused = 0, fused = 1)!");
        backward_ = mode;
    }

    // Computes the j'th self-attention head of the i'th layer (gat.hpp:83-104)
    void computeSelfAttentionHead(int i, int j) {
        DenseMatrix A;
        if (j == 0) drop_input(i);
        head_product(i, j, A, HNH_STREAM_COMPUTE);
        head_addend(i, j, HNH_STREAM_COMPUTE);
        if (score_ == HNH_GAT_SCORE_ADDITIVE) {
            shape_scored(i, scored[0]);
            head_scores(i, j, A, scored[0], HNH_STREAM_COMPUTE);
            head_attention(i, j, scored[0]);
            return;
        }
        head_attention(i, j, A);
    }

    // The reference runs the heads one after the other (gat.hpp:106-112).  Here a layer is a two-stage pipeline: the product
    // X * W of head j + 1 (MFMA bound, HNH_STREAM_AUX) runs beside the attention pass of head j (HBM bound, the compute stream),
    // between two product buffers; the layers' outputs are the reference's, bit for bit (same kernels, same operands).
    // HNH_GAT_SERIAL=1: the reference's order on one stream (A/B measurements).
    void forwardPass() {
        const bool additive = score_ == HNH_GAT_SCORE_ADDITIVE;
        check_supported(OP_FORWARD);
        if (learns_vectors())
            for (size_t i = 0; i < layers.size(); i++) ensure_attn_vectors((int)i);  // (on the compute stream, before the marks below)
        if (std::getenv("HNH_GAT_SERIAL") != nullptr) {
            for (size_t i = 0; i < layers.size(); i++) {
                shape_pre((int)i);
                for (int j = 0; j < layers[i].num_heads; j++) computeSelfAttentionHead((int)i, j);
                norm_forward((int)i);
            }
            return;
        }
        hnh::World* w = d_ops->world;
        if (!ev_input)
            for (void** e : {&ev_input, &ev_gemm[0], &ev_gemm[1], &ev_head[0], &ev_head[1]}) *e = w->event_create();
        for (size_t i = 0; i < layers.size(); i++) {
            const int H = layers[i].num_heads;
            // (allocated before the mark below: the allocator orders a recycled block behind its last use on the compute and
            // communication streams, and the auxiliary stream inherits that through the mark)
            for (int b = 0; b < (H > 1 ? 2 : 1); b++) {
                shape_product((int)i, product[b]);
                if (additive) shape_scored((int)i, scored[b]);
            }
            shape_residual((int)i);
            shape_pre((int)i);  // (a normalised layer's pre-normalisation rows: allocated before the mark below, for the same reason)
            drop_input((int)i);  // (Xd: allocated and made on the compute stream, before the mark below)
            // the layer's input is complete, and both product buffers are free, once the compute stream gets here
            w->event_record(ev_input, HNH_STREAM_COMPUTE);
            w->event_wait(ev_input, HNH_STREAM_AUX);
            head_product((int)i, 0, product[0], HNH_STREAM_AUX);
            head_addend((int)i, 0, HNH_STREAM_AUX);  // (the head's addend into its column block of buffers[i + 1]: the product stage too)
            if (additive) head_scores((int)i, 0, product[0], scored[0], HNH_STREAM_AUX);  // (the score kernel belongs to the product stage)
            w->event_record(ev_gemm[0], HNH_STREAM_AUX);
            for (int j = 0; j < H; j++) {
                w->event_wait(ev_gemm[j % 2], HNH_STREAM_COMPUTE);
                if (j + 1 < H) {
                    // product[(j + 1) % 2] was last read by head j - 1, which the compute stream has been given already
                    if (j >= 1) w->event_wait(ev_head[(j - 1) % 2], HNH_STREAM_AUX);
                    head_product((int)i, j + 1, product[(j + 1) % 2], HNH_STREAM_AUX);
                    head_addend((int)i, j + 1, HNH_STREAM_AUX);
                    if (additive) head_scores((int)i, j + 1, product[(j + 1) % 2], scored[(j + 1) % 2], HNH_STREAM_AUX);
                    w->event_record(ev_gemm[(j + 1) % 2], HNH_STREAM_AUX);
                }
                head_attention((int)i, j, additive ? scored[j % 2] : product[j % 2]);
                w->event_record(ev_head[j % 2], HNH_STREAM_COMPUTE);
            }
            norm_forward((int)i);  // (a normalised layer: pre_[i] -> buffers[i + 1] behind the last head, on the compute stream)
        }
        // every product was awaited by the compute stream: nothing is left on the auxiliary stream
        forward_valid_ = true;
    }

    // The weights or the input changed: the stored activations no longer belong to them (backwardPass refuses until a new forward).
    void invalidate_forward() { forward_valid_ = false; }

    // Gradients of L with respect to every weight matrix and the input, given G = dL/d(buffers.back()) in that buffer's layout.
    // Results: weight_grads[i] (input_features x H f of layer i, column block h = dW_h, the same on every rank) and input_grads[i]
    // (dL/d(buffers[i]); input_grads[0] is the input gradient).  Buffers are allocated on the first call and reused.
    void backwardPass(const DenseMatrix& grad_out) {
        check_supported(OP_BACKWARD);
        if (!forward_valid_) throw hnh::Error("Error, GAT backwardPass needs a forwardPass first (and a new one after set_weight / set_input)!");
        const DenseMatrix& last = buffers.back();
        if (grad_out.rows() != last.rows() || grad_out.cols() != last.cols()) throw hnh::Error("Error, GAT output gradient has the wrong shape!");
        const int L = (int)layers.size();
        if ((int)weight_grads.size() != L) {
            weight_grads.assign((size_t)L, DenseMatrix());
            input_grads.assign((size_t)L, DenseMatrix());
        }
        if (learns_vectors() && (int)attn_grads.size() != L) attn_grads.assign((size_t)L, DenseMatrix());
        if (score_ == HNH_GAT_SCORE_TRANSFORMER)
            for (auto& gq : qk_weight_grads)
                if ((int)gq.size() != L) gq.assign((size_t)L, DenseMatrix());
        if ((int)bias_grads.size() != L) {
            bias_grads.assign((size_t)L, DenseMatrix());
            res_weight_grads.assign((size_t)L, DenseMatrix());
        }
        const DenseMatrix* G = &grad_out;
        for (int i = L - 1; i >= 0; i--) {
            backward_layer(i, *G);
            G = &input_grads[(size_t)i];
        }
        grads_fresh_ = true;  // (optimizer_step takes them once)
    }

    // The attention coefficients of (layer i, head h) of the STORED forward pass, one per nonzero of S on this rank, into `out` in the
    // like_S_values layout (Distributed_Sparse::S_coordinates gives the global (row, column) of every entry): a_ij = exp(z_ij - lse_i) with
    // the lse the forward pass kept, normalised over ALL edges of the row.  `dropped` with a nonzero attention rate: c m_ij a_ij instead, the
    // weights the aggregate actually used (rate 0: no difference).  One pass over the nonzeros (include/hnh_attn_coef.h): A = layer_input(i)
    // W_h is recomputed (Xd under feature dropout, what the forward pass used); the scores dot and gatv2 gather A, score additive gathers
    // the packed pair [t | id] built from A, and the schedule runs at that operand's width and at its previous R again afterwards.  Reads
    // the stored pass and writes `out` and scratch of its own: buffers, lse, gradients, seed and optimizer state stay as they are, and so
    // does the validity of the forward pass.  Attention softmax on 15d_fusion2 with c = 1 and heads of at most HNH_ATTN_COEF_MAX_F
    // features; everything else raises before anything is launched (arguments, mode, schedule, width, kernel group, then the stored pass).
    void attention_coefficients(int i, int h, VectorXd& out, bool dropped) {
        const std::string what = "attention_coefficients";
        check_layer_head(i, h);
        if (score_ == HNH_GAT_SCORE_TRANSFORMER)
            throw hnh::Error("Error, GAT " + what + " does not support score transformer: the export has no query/key/value pass (include/hnh_attn_coef.h)");
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);
        if (ds != nullptr) {
            SpmatLocal* s = ds->fusionApproach == 1 ? ds->ST.get() : ds->S.get();
            const int64_t want = (int64_t)(s->owned_coords_end - s->owned_coords_start);
            if (out.size() != want)
                throw hnh::Error("Error, GAT " + what + " needs a vector of like_S_values length: " + std::to_string(want) + " entries, not " +
                                 std::to_string(out.size()) + "!");
        }
        require_softmax(what, ": its weights are what sddmmA and hnh_leaky_relu_f64 give", "include/hnh_attn_coef.h");
        require_own_rows(what);
        require_head_width(what, HNH_ATTN_COEF_MAX_F, "include/hnh_attn_coef.h", i);
        GATLayer& L = layers[(size_t)i];
        const int f = L.features_per_head;
        const bool additive = score_ == HNH_GAT_SCORE_ADDITIVE;
        require_kernels(what, {HNH_GAT_KERNEL(hnh_attn_coef_csr_p)});
        if (additive) require_kernels(what, {HNH_GAT_KERNEL(hnh_attn_coef_scores_f64)});
        if (!forward_valid_ || lse_.size() != layers.size() || lse_[(size_t)i].size() != (size_t)L.num_heads)
            throw hnh::Error("Error, GAT " + what + " needs a forwardPass first (and a new one after set_weight / set_input / optimizer_step)!");
        const int S0 = HNH_STREAM_COMPUTE;
        DenseMatrix& X = layer_input(i);
        const int64_t rows = X.rows();
        DenseMatrix& A = scratch(SC_COEF_A, rows, f);
        HNH_GAT_CALL(hnh_gemm_f64, rows, f, X.cols(), X.data(), L.wMats[(size_t)h].data(), A.data(), S0);
        hnh_attn_coef g = {};
        g.lse = lse_[(size_t)i][(size_t)h].data();
        g.f = f;
        g.leaky_alpha = leaky_relu_alpha;
        const int r0 = d_ops->R;
        bool ok;
        if (additive) {
            DenseMatrix& sv = scratch(SC_COEF_S, rows, 1);
            DenseMatrix& T = scratch(SC_COEF_T, rows, HNH_ATTN_COEF_PAIR_WIDTH);
            HNH_GAT_CALL(hnh_attn_coef_scores_f64, sv.data(), T.data(), T.cols(), A.data(), f, attn_vector(i, h, 0), attn_vector(i, h, 1), rows, f,
                         d_ops->aSubmatrices[0].topRow, S0);
            g.score = HNH_ATTN_COEF_ADDITIVE;
            g.s = sv.data();
            const bool drop = dropped && attn_p_ > 0.0;
            const hnh_attn_drop dr = attn_drop_args(i, h);
            ScheduleWidth width(d_ops, HNH_ATTN_COEF_PAIR_WIDTH, r0);
            hnh::AttnPass pass = {0, g, drop ? &dr : nullptr};
            pass.coef = &out;
            ok = ds->attn_pass(pass, T, rows, false);
        } else {
            g.score = score_ == HNH_GAT_SCORE_GATV2 ? HNH_ATTN_COEF_GATV2 : HNH_ATTN_COEF_DOT;
            g.X = A.data();
            g.ld_x = f;
            g.a = score_ == HNH_GAT_SCORE_GATV2 ? attn_vector(i, h, 0) : nullptr;
            ScheduleWidth width(d_ops, f, r0);
            hnh::AttnPass pass = {0, g};
            pass.coef = &out;
            ok = ds->attn_pass(pass, A, rows, false);
        }
        require_own_rows(what, !ok);
    }

    // ---- training (include/hnh_train.h)
    // Labels and training mask as HOST arrays of d_ops->M entries in the operator's global row numbering (mask == nullptr: every row with
    // a label >= 0).  heads_mode: HNH_GAT_HEADS_MEAN (classes = the last layer's features_per_head) | HNH_GAT_HEADS_CONCAT (classes =
    // num_heads * features_per_head).  Collective: the labelled count is summed over the world.
    void set_labels(const int32_t* labels, const uint8_t* mask, int64_t n, int heads_mode) {
        if (heads_mode != HNH_GAT_HEADS_MEAN && heads_mode != HNH_GAT_HEADS_CONCAT)
            throw hnh::Error("Error, unknown GAT label heads mode " + std::to_string(heads_mode) + " (mean = 0, concat = 1)!");
        if (labels == nullptr) throw hnh::Error("Error, GAT set_labels: null labels!");
        if (n != d_ops->M)
            throw hnh::Error("Error, GAT set_labels needs one label per global row: " + std::to_string(d_ops->M) + " entries, not " + std::to_string(n) + "!");
        check_whole_rows("set_labels");
        std::vector<int32_t> keep_labels(labels, labels + n);
        std::vector<uint8_t> keep_mask;
        if (mask) keep_mask.assign(mask, mask + n);
        const int old_mode = label_heads_;
        label_heads_ = heads_mode;
        try {
            labels_host_.swap(keep_labels);
            train_set_ = make_label_set(keep_mask.empty() ? nullptr : keep_mask.data());
        } catch (...) {
            labels_host_.swap(keep_labels);  // a refused call leaves the object as it was
            label_heads_ = old_mode;
            throw;
        }
        train_mask_.swap(keep_mask);
        labels_set_ = true;
        multilabel_ = false;  // the most recent of set_labels / set_multilabel_targets decides the head
    }

    // ---- the multi-label head (include/hnh_train_multilabel.h)
    // Targets as a HOST array of d_ops->M x classes values in {0, 1} (row-major, the operator's global row numbering), a training mask of
    // mask_n = d_ops->M bytes (nullptr: every row) and `classes` class weights (nullptr: every weight 1; the pos_weight of the weighted
    // sigmoid cross-entropy).  classes must be what heads_mode gives: the last layer's features_per_head (MEAN) or num_heads *
    // features_per_head (CONCAT).  Afterwards loss / train_step / evaluate use the sigmoid head: the loss is the mean over selected rows x
    // classes, the pair's second value micro-F1.  Each rank packs its own rows' bits and keeps them with its rows of the mask on the device.
    // Collective: the selected row count is summed over the world.  Every refusal comes before anything is launched and leaves the object
    // as it was.
    void set_multilabel_targets(const uint8_t* targets, int64_t n, int classes, const uint8_t* mask, int64_t mask_n, int heads_mode,
                                const double* pos_weight) {
        if (heads_mode != HNH_GAT_HEADS_MEAN && heads_mode != HNH_GAT_HEADS_CONCAT)
            throw hnh::Error("Error, unknown GAT label heads mode " + std::to_string(heads_mode) + " (mean = 0, concat = 1)!");
        if (targets == nullptr) throw hnh::Error("Error, GAT set_multilabel_targets: null targets!");
        const int want = classes_of(heads_mode);
        if (classes != want)
            throw hnh::Error("Error, GAT set_multilabel_targets: " + std::to_string(classes) + " classes, but heads mode " + std::to_string(heads_mode) +
                             " of the last layer gives " + std::to_string(want) + "!");
        const int64_t M = d_ops->M;
        if (n != M * classes)
            throw hnh::Error("Error, GAT set_multilabel_targets needs " + std::to_string(M) + " x " + std::to_string(classes) + " = " + std::to_string(M * classes) +
                             " targets, not " + std::to_string(n) + "!");
        if (mask != nullptr && mask_n != M)
            throw hnh::Error("Error, GAT set_multilabel_targets: the mask needs " + std::to_string(M) + " entries, not " + std::to_string(mask_n) + "!");
        check_whole_rows("set_multilabel_targets");
        for (int64_t i = 0; i < n; i++)
            if (targets[i] > 1)
                throw hnh::Error("Error, GAT multi-label target " + std::to_string((int)targets[i]) + " of row " + std::to_string(i / classes) + ", class " +
                                 std::to_string(i % classes) + " is neither 0 nor 1!");
        for (int c = 0; pos_weight != nullptr && c < classes; c++)
            if (!(pos_weight[c] >= 0.0) || !std::isfinite(pos_weight[c]))
                throw hnh::Error("Error, GAT multi-label pos_weight " + std::to_string(pos_weight[c]) + " of class " + std::to_string(c) +
                                 " is negative or not finite!");
        // the new state in temporaries: a refusal of make_target_set leaves the object as it was
        TargetSet set = make_target_set(mask);
        hnh::World* w = d_ops->world;
        const int64_t rows = buffers.back().rows(), top = d_ops->aSubmatrices[0].topRow, words = ((int64_t)classes + 31) / 32;
        std::vector<uint32_t> bits((size_t)(rows * words), 0u);
        for (int64_t r = 0; r < rows && top + r < M; r++)
            for (int c = 0; c < classes; c++)
                if (targets[(top + r) * classes + c]) bits[(size_t)(r * words + c / 32)] |= 1u << (c % 32);
        hnh::DeviceArray dbits(w, (size_t)(rows * words) * sizeof(uint32_t));
        if (rows > 0) w->copy(dbits.ptr(), bits.data(), (size_t)(rows * words) * sizeof(uint32_t), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        DenseMatrix weights;
        if (pos_weight != nullptr) {
            weights = DenseMatrix(classes, 1);
            w->copy(weights.data(), pos_weight, (size_t)classes * sizeof(double), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        }
        w->sync(HNH_STREAM_COMPUTE);  // (`bits` and the caller's weights have been read)
        ml_bits_ = std::move(dbits);
        ml_weights_ = std::move(weights);
        ml_train_set_ = std::move(set);
        ml_words_ = words;
        ml_heads_ = heads_mode;
        ml_counts_[0] = ml_counts_[1] = ml_counts_[2] = 0.0;
        multilabel_ = true;
    }
    // (tp, fp, fn) of the last loss / evaluate / train_step under the sigmoid head, summed over the world: counts of (row, class) pairs
    void multilabel_counts(double* tp, double* fp, double* fn) const {
        if (!multilabel_) throw hnh::Error("Error, GAT multilabel_counts needs set_multilabel_targets first (and no set_labels since)!");
        *tp = ml_counts_[0];
        *fp = ml_counts_[1];
        *fn = ml_counts_[2];
    }

    // (loss, accuracy) of the stored forward pass over the rows of `mask` (HOST, global numbering; nullptr: the training rows of set_labels);
    // grad_out != nullptr also receives dL/d(output) in the last buffer's layout, which backwardPass takes.  Collective.
    std::pair<double, double> loss(const uint8_t* mask, int64_t n, DenseMatrix* grad_out) {
        check_supported(OP_LOSS);
        if (!forward_valid_) throw hnh::Error("Error, GAT loss needs a forwardPass first (and a new one after set_weight / set_input / optimizer_step)!");
        if (mask != nullptr && n != d_ops->M) throw hnh::Error("Error, GAT loss: the mask needs " + std::to_string(d_ops->M) + " entries, not " + std::to_string(n) + "!");
        const DenseMatrix& last = buffers.back();
        if (grad_out != nullptr && (grad_out->rows() != last.rows() || grad_out->cols() != last.cols()))
            throw hnh::Error("Error, GAT loss: the output gradient has the wrong shape!");
        if (multilabel_) {  // (loss, micro-F1) of the sigmoid head
            TargetSet other_rows;
            if (mask != nullptr) other_rows = make_target_set(mask);
            const TargetSet& ts = mask != nullptr ? other_rows : ml_train_set_;
            bce_enqueue(ts, grad_out);
            return bce_read(ts);
        }
        LabelSet other;
        if (mask != nullptr) other = make_label_set(mask);
        const LabelSet& ls = mask != nullptr ? other : train_set_;
        loss_enqueue(ls, grad_out);
        return loss_read(ls);
    }

    // Sets the hyper-parameters, drops every moment and resets the step count.  kind: HNH_OPTIM_ADAM | HNH_OPTIM_SGD (include/hnh_train.h) |
    // HNH_OPTIM_ADAMW (include/hnh_train_clip.h).  The clip setting (set_grad_clip) and the schedule (set_lr_schedule) stay in place; lr
    // becomes the schedule's base rate.
    void set_optimizer(int kind, double lr, double beta1, double beta2, double eps, double momentum, double weight_decay) {
        if (kind != HNH_OPTIM_ADAM && kind != HNH_OPTIM_SGD && kind != HNH_OPTIM_ADAMW)
            throw hnh::Error("Error, unknown GAT optimizer " + std::to_string(kind) + " (adam = 0, sgd = 1, adamw = 2)!");
        if (!(lr >= 0.0) || !std::isfinite(lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(momentum >= 0.0 && momentum < 1.0) ||
            !(weight_decay >= 0.0) || !std::isfinite(weight_decay) || !std::isfinite(eps))
            throw hnh::Error("Error, GAT set_optimizer needs lr, eps, weight_decay >= 0 and beta1, beta2, momentum in [0, 1)!");
        optim_ = {};
        optim_.kind = kind;
        optim_.lr = lr;
        optim_.beta1 = beta1;
        optim_.beta2 = beta2;
        optim_.eps = eps;
        optim_.momentum = momentum;
        optim_.weight_decay = weight_decay;
        moments_.clear();
        optim_steps_ = 0;
        optimizer_set_ = true;
    }
    int64_t optimizer_steps() const { return optim_steps_; }

    // ---- gradient clipping, learning rate and schedule (include/hnh_train_clip.h)
    // Clipping by global norm: every later optimizer_step / train_step scales all gradients by min(1, max_norm / (norm + 1e-6)), norm =
    // the 2-norm over every learned tensor of the whole world (torch.nn.utils.clip_grad_norm_).  0 switches it off (the default).
    void set_grad_clip(double max_norm) {
        if (!(max_norm >= 0.0) || !std::isfinite(max_norm))
            throw hnh::Error("Error, GAT set_grad_clip needs a finite max_norm >= 0 (0: no clipping), not " + std::to_string(max_norm) + "!");
        clip_max_ = max_norm;
    }
    // The global gradient norm, before clipping, of the most recent clipped optimizer_step / train_step: a copy and a host synchronisation
    // of its own.
    double grad_norm() {
        if (clip_nsums_ == 0) throw hnh::Error("Error, GAT grad_norm needs an optimizer_step or train_step with clipping switched on (set_grad_clip) first!");
        hnh::World* w = d_ops->world;
        double s[2] = {0.0, 0.0};
        w->copy(s, clip_sums_.data(), sizeof(double) * (size_t)clip_nsums_, HNH_COPY_D2H, HNH_STREAM_COMPUTE);
        w->sync(HNH_STREAM_COMPUTE);
        double total = 0.0;
        for (int q = 0; q < clip_nsums_; q++) total += s[q];  // (the kernel's sum)
        return std::sqrt(total);
    }
    // A new base rate; moments and step count stay.
    void set_learning_rate(double lr) {
        if (!optimizer_set_) throw hnh::Error("Error, GAT set_learning_rate needs set_optimizer first!");
        if (!(lr >= 0.0) || !std::isfinite(lr)) throw hnh::Error("Error, GAT set_learning_rate needs a finite lr >= 0!");
        optim_.lr = lr;
    }
    // lr_t = lr * factor(t) for the 1-based step t: t / W during a warm-up of W steps; then 1 (HNH_GAT_LR_CONSTANT, which ignores total and
    // min_factor), or a linear / cosine descent to min_factor at step T = total, and min_factor from there on.
    void set_lr_schedule(int kind, int64_t warmup, int64_t total, double min_factor) {
        if (kind != HNH_GAT_LR_CONSTANT && kind != HNH_GAT_LR_LINEAR && kind != HNH_GAT_LR_COSINE)
            throw hnh::Error("Error, unknown GAT learning-rate schedule " + std::to_string(kind) + " (constant = 0, linear = 1, cosine = 2)!");
        if (warmup < 0 || total < 0 || !(min_factor >= 0.0 && min_factor <= 1.0))
            throw hnh::Error("Error, GAT set_lr_schedule needs warmup_steps >= 0, total_steps >= 0 and min_factor in [0, 1]!");
        if (kind != HNH_GAT_LR_CONSTANT && total <= warmup)
            throw hnh::Error("Error, GAT set_lr_schedule: a linear or cosine schedule needs total_steps > warmup_steps, not " + std::to_string(total) + " and " +
                             std::to_string(warmup) + "!");
        sched_kind_ = kind;
        sched_warmup_ = warmup;
        sched_total_ = total;
        sched_min_ = min_factor;
    }
    double lr_factor(int64_t t) const {
        const double W = (double)sched_warmup_, T = (double)sched_total_, x = (double)t;
        if (t <= sched_warmup_) return x / W;
        if (sched_kind_ == HNH_GAT_LR_CONSTANT) return 1.0;
        if (t > sched_total_) return sched_min_;
        const double s = (x - W) / (T - W);
        if (sched_kind_ == HNH_GAT_LR_LINEAR) return 1.0 - (1.0 - sched_min_) * s;
        return sched_min_ + (1.0 - sched_min_) * 0.5 * (1.0 + std::cos(3.14159265358979323846 * s));
    }
    // the rate of the next step
    double learning_rate() const {
        if (!optimizer_set_) throw hnh::Error("Error, GAT learning_rate needs set_optimizer first!");
        return optim_.lr * lr_factor(optim_steps_ + 1);
    }

    // One optimizer step from the gradients of the last backwardPass over learned_parameters(), in one table.  Invalidates the stored
    // forward pass.  No host synchronisation.  With clipping off and kind Adam or SGD: hnh_optim_step_f64, as ever.  With clipping on:
    // hnh_grad_sumsq_f64 first, the replicated tensors into sums[0] (their gradients are bit-equal on every rank: no collective) and the
    // S-order copy of every learned edge bias, which each rank holds for its own nonzeros, into sums[1], summed over the world; then both
    // tables through hnh_optim_step_clip_f64 with the two sums, so every rank takes the same coefficient.  Kind AdamW always takes that
    // entry point (a null sumsq without clipping).
    void optimizer_step() {
        if (!optimizer_set_) throw hnh::Error("Error, GAT optimizer_step needs set_optimizer first!");
        require_kernels("training", {HNH_GAT_KERNEL(hnh_optim_step_f64)});
        require_clip_kernels();
        if (!grads_fresh_ || weight_grads.size() != layers.size() || (learns_vectors() && attn_grads.size() != layers.size()))
            throw hnh::Error("Error, GAT optimizer_step needs the gradients of a backwardPass since the last step!");
        const std::vector<Learned> learned = learned_parameters();
        for (const Learned& t : learned)
            if (t.g == nullptr) throw hnh::Error(t.refusal);
        // the learned edge biases (PARAM_EDGE_BIAS_S / _ST) and the norms' gamma and beta (PARAM_NORM_GAIN / _SHIFT) in a table and a call of
        // their own: they are never decayed
        std::vector<hnh_optim_tensor> table, undecayed, replicated, per_rank;  // (the last two: what the norm is made of)
        bool edge_learned = false;
        for (const Learned& t : learned) {
            const int kind = std::get<0>(t.key);
            edge_learned = edge_learned || kind == PARAM_EDGE_BIAS_S;
            if (t.rows == 0) continue;  // (a rank without nonzeros holds none of a layer's bias)
            const Moments& m = ensure_moments(t);
            const bool edge = kind == PARAM_EDGE_BIAS_S || kind == PARAM_EDGE_BIAS_ST || kind == PARAM_NORM_GAIN || kind == PARAM_NORM_SHIFT;
            (edge ? undecayed : table).push_back({t.p, t.ld_p, t.g, t.ld_g, m.first.data(), m.second.data(), t.rows, t.cols});
            // the S^T-order copy of an edge bias holds the numbers of the S-order one: counted once
            if (kind == PARAM_EDGE_BIAS_S) per_rank.push_back((edge ? undecayed : table).back());
            else if (kind != PARAM_EDGE_BIAS_ST) replicated.push_back((edge ? undecayed : table).back());
        }
        const bool clip = clip_max_ > 0.0, through_clip = clip || optim_.kind == HNH_OPTIM_ADAMW;
        const int nsums = edge_learned ? 2 : 1;
        if (clip) {
            if (clip_sums_.size() != 2) clip_sums_ = DenseMatrix(2, 1);
            const std::vector<hnh_optim_tensor>* part[2] = {&replicated, &per_rank};
            for (int q = 0; q < nsums; q++) {
                const int64_t need = d_ops->world->be->hnh_grad_sumsq_f64_workspace(part[q]->data(), (int)part[q]->size());
                if (need < 0) throw hnh::Error("Error, GAT optimizer_step: a gradient has a shape that hnh_grad_sumsq_f64 refuses!");
                DenseMatrix& work = scratch(SC_SUMSQ_WORK, need, 1);
                HNH_GAT_CALL(hnh_grad_sumsq_f64, part[q]->data(), (int)part[q]->size(), 0, clip_sums_.data() + q, work.data(), need, HNH_STREAM_COMPUTE);
            }
            if (edge_learned) sum_over_world(clip_sums_.data() + 1, 1);
            clip_nsums_ = nsums;
        }
        optim_steps_++;
        hnh_optim hy = optim_;
        hy.lr = optim_.lr * lr_factor(optim_steps_);  // (factor 1.0 without a schedule: the same bits)
        hy.bias1 = 1.0 - std::pow(hy.beta1, (double)optim_steps_);
        hy.bias2 = 1.0 - std::pow(hy.beta2, (double)optim_steps_);
        const double* sums = clip ? clip_sums_.data() : nullptr;
        if (through_clip) HNH_GAT_CALL(hnh_optim_step_clip_f64, table.data(), (int)table.size(), &hy, sums, nsums, clip_max_, HNH_STREAM_COMPUTE);
        else HNH_GAT_CALL(hnh_optim_step_f64, table.data(), (int)table.size(), &hy, HNH_STREAM_COMPUTE);
        if (!undecayed.empty()) {
            hy.weight_decay = 0.0;
            if (through_clip) HNH_GAT_CALL(hnh_optim_step_clip_f64, undecayed.data(), (int)undecayed.size(), &hy, sums, nsums, clip_max_, HNH_STREAM_COMPUTE);
            else HNH_GAT_CALL(hnh_optim_step_f64, undecayed.data(), (int)undecayed.size(), &hy, HNH_STREAM_COMPUTE);
        }
        grads_fresh_ = false;
        invalidate_forward();
    }

    // One training step; returns (loss, accuracy) over the training rows, of the parameters before the update.  With a nonzero dropout
    // rate the seed advances by one first, so step t of a run uses the masks of seed0 + t.
    std::pair<double, double> train_step() {
        check_supported(OP_TRAIN_STEP);
        const uint64_t seed0 = seed_;
        const int64_t steps0 = optim_steps_;
        if (attn_p_ > 0.0 || feat_p_ > 0.0) seed_ += 1;  // (mod 2^64)
        try {
            forwardPass();
            const DenseMatrix& last = buffers.back();
            if (train_grad_.rows() != last.rows() || train_grad_.cols() != last.cols()) train_grad_ = DenseMatrix(last.rows(), last.cols());
            if (multilabel_) bce_enqueue(ml_train_set_, &train_grad_);
            else loss_enqueue(train_set_, &train_grad_);
            backwardPass(train_grad_);
            optimizer_step();
        } catch (...) {  // (a step that did not update leaves seed and step count as they were: step t keeps seed0 + t)
            if (optim_steps_ == steps0) seed_ = seed0;
            throw;
        }
        return multilabel_ ? bce_read(ml_train_set_) : loss_read(train_set_);
    }

    // (loss, accuracy) over the rows of `mask` (nullptr: the training rows) from a forward pass without dropout and without a gradient.
    // Rates and seed are as before afterwards; the stored forward pass is valid only if both rates were 0.
    std::pair<double, double> evaluate(const uint8_t* mask, int64_t n) {
        check_supported(OP_EVALUATE);
        if (mask != nullptr && n != d_ops->M) throw hnh::Error("Error, GAT evaluate: the mask needs " + std::to_string(d_ops->M) + " entries, not " + std::to_string(n) + "!");
        LabelSet other;
        TargetSet other_rows;
        if (mask != nullptr && multilabel_) other_rows = make_target_set(mask);
        else if (mask != nullptr) other = make_label_set(mask);
        const LabelSet& ls = mask != nullptr ? other : train_set_;
        const TargetSet& ts = mask != nullptr ? other_rows : ml_train_set_;
        const double ap = attn_p_, fp = feat_p_;
        attn_p_ = feat_p_ = 0.0;
        std::pair<double, double> res;
        try {
            forwardPass();
            if (multilabel_) {
                bce_enqueue(ts, nullptr);
                res = bce_read(ts);
            } else {
                loss_enqueue(ls, nullptr);
                res = loss_read(ls);
            }
        } catch (...) {
            attn_p_ = ap;
            feat_p_ = fp;
            invalidate_forward();
            throw;
        }
        attn_p_ = ap;
        feat_p_ = fp;
        if (ap > 0.0 || fp > 0.0) invalidate_forward();
        return res;
    }

    void get_weight(int i, int h, double* host) {
        check_layer_head(i, h);
        layers[(size_t)i].wMats[(size_t)h].copy_to_host(host);
    }
    void get_attn_vectors(int i, int h, double* a1_host, double* a2_host) {
        check_layer_head(i, h);
        ensure_attn_vectors(i);
        d_ops->world->sync_all();
        copy_attn_vectors(i, h, a1_host, a2_host, HNH_COPY_D2H);
    }

    std::vector<DenseMatrix> weight_grads, input_grads;
    // score ADDITIVE: attn_grads[i] is (num_heads * features_per_head) x 2 of layer i, row h f + c = (da1_h[c], da2_h[c]), the same on every rank;
    // score GATV2: the same shape, row h f + c = (da_h[c], 0)
    std::vector<DenseMatrix> attn_grads;
    // bias_grads[i] ((num_heads * features_per_head) x 1, a layer with a bias) and res_weight_grads[i] (input_features x (num_heads *
    // features_per_head), residual projection) of layer i, the same on every rank; empty for a layer without
    std::vector<DenseMatrix> bias_grads, res_weight_grads;
    // score TRANSFORMER: qk_weight_grads[0][i] = dW_q and [1][i] = dW_k of layer i (input_features x (num_heads * features_per_head), column
    // block h belongs to head h, like weight_grads), the same on every rank
    std::vector<DenseMatrix> qk_weight_grads[2];

private:
    hnh::World* world_ = nullptr;
    bool forward_valid_ = false;
    int attention_ = HNH_GAT_ATTENTION_NONE;
    int backward_ = HNH_GAT_BACKWARD_UNFUSED;
    int score_ = HNH_GAT_SCORE_DOT;
    double attn_p_ = 0.0, feat_p_ = 0.0;  // dropout rates and the masks' seed (include/hnh_attn_dropout.h)
    uint64_t seed_ = 0;
    std::vector<int> act_;                // HNH_GAT_ACT_* of every layer's output
    DenseMatrix act_delta_;               // the delta of the head in hand where one launch makes dZ and delta: head_dz writes it, head_delta hands it out
    std::vector<DenseMatrix> xd_;         // feature dropout: Xd of every layer (allocated only then)
    // bias and skip connections (include/hnh_gat_skip.h): per layer the residual mode, W_res per head (input_features x f each, the
    // contiguous operand of hnh_gemm_f64; projection only), the bias (H f x 1) with its enabled bit; the projection of the head in
    // flight (the auxiliary stream's scratch)
    std::vector<int> res_mode_;
    std::vector<char> bias_on_;
    std::vector<DenseMatrix> bias_;
    std::vector<std::vector<DenseMatrix>> w_res_;
    DenseMatrix res_product_;
    // layer normalisation (include/hnh_gat_norm.h): per layer the mode and eps, gamma and beta (H f x 1 each, allocated when the layer is
    // first normalised or its weights are set), [dgamma; dbeta] (2 x H f) with whether a backward pass has filled it since the layer's norm
    // last changed, and of the stored forward pass the pre-normalisation rows z (rows x H f) and the rows' (mu, 1 / sigma) (rows x 2)
    std::vector<int> norm_;
    std::vector<double> norm_eps_;
    std::vector<DenseMatrix> norm_gain_, norm_shift_, norm_grads_, pre_, norm_stats_;
    std::vector<char> norm_grads_held_;
    // the per-edge bias (include/hnh_attn_edge.h) of every layer: [0] in S's order, [1] in S^T's, with its enabled bit (kept here, not in
    // GATLayer, for act_'s reason)
    std::vector<char> edge_bias_on_;
    std::vector<VectorXd> edge_bias_[2];
    int64_t edge_len_[2] = {-1, -1};  // the lengths of like_S_values / like_ST_values, once set_edge_bias has asked for them
    // a learned edge bias (include/hnh_attn_edge_grad.h): the switch per layer, dL/db in both orders ([0]: S's, from the row pass; [1]:
    // S^T's, from the column pass) and whether a backward pass has filled them since they were last dropped
    std::vector<char> edge_bias_learned_, dbias_held_;
    std::vector<VectorXd> dbias_[2];
    void drop_edge_bias_grad(int i) {
        dbias_held_[(size_t)i] = 0;
        for (auto& e : dbias_) e[(size_t)i] = VectorXd();
    }
    void check_edge_which(int i, int which) const {
        check_layer(i);
        if (which != 0 && which != 1) throw hnh::Error("Error, GAT edge-bias order selector " + std::to_string(which) + " is neither 0 (S) nor 1 (S^T)!");
    }
    void copy_edge_vector(const VectorXd& from, VectorXd& out, const char* who) {
        if (out.size() != from.size())
            throw hnh::Error(std::string("Error, GAT ") + who + " needs a vector of " + std::to_string(from.size()) + " entries, not " + std::to_string(out.size()) + "!");
        if (from.size() > 0) d_ops->world->copy(out.data(), from.data(), sizeof(double) * (size_t)from.size(), HNH_COPY_D2D, HNH_STREAM_COMPUTE);
    }
    // score TRANSFORMER: W_q ([0]) and W_k ([1]) per (layer, head), input_features x f each (kept here, not in GATLayer, for act_'s reason)
    std::vector<std::vector<DenseMatrix>> w_qk_[2];
    // training (include/hnh_train.h): this rank's labels on the device (-1: not in the loss) with the world's labelled count; the host's
    // copy of all labels and of the training mask (loss / evaluate build other sets from them); the optimizer and its moments
    struct LabelSet {
        hnh::DeviceArray labels;
        double count = 0.0;
    };
    bool labels_set_ = false, optimizer_set_ = false, grads_fresh_ = false;
    int label_heads_ = HNH_GAT_HEADS_MEAN;
    std::vector<int32_t> labels_host_;
    std::vector<uint8_t> train_mask_;
    LabelSet train_set_;
    DenseMatrix train_grad_, loss_result_;
    // the multi-label head (include/hnh_train_multilabel.h): whether it is the head in use (the most recent of set_labels /
    // set_multilabel_targets decides), this rank's rows of the bit-packed targets (ml_words_ words a row) and of a mask with the world's
    // selected row count, the class weights (empty: none), the heads mode, and (tp, fp, fn) of the last loss
    struct TargetSet {
        hnh::DeviceArray mask;
        double count = 0.0;
    };
    bool multilabel_ = false;
    int ml_heads_ = HNH_GAT_HEADS_MEAN;
    int64_t ml_words_ = 0;
    hnh::DeviceArray ml_bits_;
    DenseMatrix ml_weights_, ml_result_;
    TargetSet ml_train_set_;
    double ml_counts_[3] = {0.0, 0.0, 0.0};
    hnh_optim optim_ = {};
    int64_t optim_steps_ = 0;
    // gradient clipping and the schedule (include/hnh_train_clip.h): max_norm (0: off); the sums of squares of the last clipped step on the
    // device ([0]: the replicated tensors, [1]: the learned edge biases over the world) and how many of them it used (0: no clipped step
    // yet); the schedule of set_lr_schedule over optim_.lr, the base rate
    double clip_max_ = 0.0;
    DenseMatrix clip_sums_;
    int clip_nsums_ = 0;
    int sched_kind_ = HNH_GAT_LR_CONSTANT;
    int64_t sched_warmup_ = 0, sched_total_ = 0;
    double sched_min_ = 0.0;
    // Every learned tensor of the model is one row of optimizer_step's table (learned_parameters()); its moments live under its key.
    enum ParamKind { PARAM_W, PARAM_A1, PARAM_A2, PARAM_BIAS, PARAM_W_RES, PARAM_W_Q, PARAM_W_K, PARAM_EDGE_BIAS_S, PARAM_EDGE_BIAS_ST,
                     PARAM_NORM_GAIN, PARAM_NORM_SHIFT };
    typedef std::tuple<int, int, int> ParamKey;            // (kind, layer, head; head 0 for a tensor of the whole layer)
    typedef std::pair<DenseMatrix, DenseMatrix> Moments;   // (first moment: Adam only, SGD keeps none; second moment, or SGD's momentum buffer)
    struct Learned {
        ParamKey key;
        double* p;        // the value, rows x cols at pitch ld_p
        int64_t ld_p;
        const double* g;  // its gradient at pitch ld_g; nullptr where the gradient container does not hold it: `refusal` says so
        int64_t ld_g, rows, cols;
        const char* refusal;
    };
    std::map<ParamKey, Moments> moments_;

    // The table's rows in order: per layer W_0 .. W_{H-1}, then a1, then a2 (score ADDITIVE; GATV2 learns a1 alone); after all layers, per
    // layer the enabled bias, then W_res_0 .. W_res_{H-1} of a projection (include/hnh_gat_skip.h), then with score TRANSFORMER W_q_0 ..
    // W_q_{H-1} and W_k_0 .. W_k_{H-1}, then a learned edge bias in S's and in S^T's order (one nnz x 1 tensor each, behind every other
    // entry of the layer), then gamma and beta of a normalised layer (PARAM_NORM_GAIN / _SHIFT, H f x 1 each, behind every other entry of the
    // layer).  Weight decay applies to all alike but the edge bias, gamma and beta, which optimizer_step never decays (undecayed()).
    std::vector<Learned> learned_parameters() {
        std::vector<Learned> all;
        const size_t n = layers.size();
        // grads[i] where the container holds a rows x cols gradient of layer i
        auto held = [&](const std::vector<DenseMatrix>& grads, size_t i, int64_t rows, int64_t cols) -> const DenseMatrix* {
            return grads.size() == n && grads[i].rows() == rows && grads[i].cols() == cols ? &grads[i] : nullptr;
        };
        // one row: the gradient is the block of `grad` that starts at its column `at`
        auto add = [&](int kind, size_t i, int h, double* p, int64_t ld_p, int64_t rows, int64_t cols, const DenseMatrix* grad, int64_t at, const char* refusal) {
            all.push_back({ParamKey(kind, (int)i, h), p, ld_p, grad ? grad->data() + at : nullptr, grad ? grad->cols() : 0, rows, cols, refusal});
        };
        for (size_t i = 0; i < n; i++) {
            GATLayer& L = layers[i];
            const int64_t f = L.features_per_head, hf = (int64_t)L.num_heads * f;
            for (int h = 0; h < L.num_heads; h++) {
                DenseMatrix& W = L.wMats[(size_t)h];
                add(PARAM_W, i, h, W.data(), f, W.rows(), f, W.cols() == f ? held(weight_grads, i, W.rows(), hf) : nullptr, (int64_t)h * f,
                    "Error, GAT optimizer_step: a weight gradient has the wrong shape!");
            }
            if (!learns_vectors()) continue;
            ensure_attn_vectors((int)i);
            const DenseMatrix* da = held(attn_grads, i, hf, 2);  // (hf x 2: da1 and da2 interleaved; score GATV2: da and zeros)
            const char* refusal = "Error, GAT optimizer_step: an attention-vector gradient has the wrong shape!";
            add(PARAM_A1, i, 0, L.a1.data(), 1, hf, 1, da, 0, refusal);
            if (score_ == HNH_GAT_SCORE_ADDITIVE) add(PARAM_A2, i, 0, L.a2.data(), 1, hf, 1, da, 1, refusal);
        }
        for (size_t i = 0; i < n; i++) {
            const GATLayer& L = layers[i];
            const int64_t f = L.features_per_head, hf = (int64_t)L.num_heads * f, k = L.input_features;
            if (bias_on_[i])
                add(PARAM_BIAS, i, 0, bias_[i].data(), 1, hf, 1, held(bias_grads, i, hf, 1), 0,
                    "Error, GAT optimizer_step needs the bias gradient of a backwardPass since set_bias!");
            if (res_mode_[i] == HNH_GAT_RESIDUAL_PROJECTION)
                for (int h = 0; h < L.num_heads; h++)
                    add(PARAM_W_RES, i, h, w_res_[i][(size_t)h].data(), f, k, f, held(res_weight_grads, i, k, hf), (int64_t)h * f,
                        "Error, GAT optimizer_step needs the residual-weight gradient of a backwardPass since set_residual!");
            if (score_ == HNH_GAT_SCORE_TRANSFORMER) {
                ensure_qk_weights((int)i);
                for (int which = 0; which < 2; which++)
                    for (int h = 0; h < L.num_heads; h++)
                        add(which == 0 ? PARAM_W_Q : PARAM_W_K, i, h, w_qk_[which][i][(size_t)h].data(), f, k, f, held(qk_weight_grads[which], i, k, hf),
                            (int64_t)h * f, "Error, GAT optimizer_step needs the query and key weight gradients of a backwardPass with score transformer!");
                for (int which = 0; which < 2 && edge_bias_learned_[i]; which++) {
                    VectorXd& b = edge_bias_[which][i];
                    const VectorXd& g = dbias_[which][i];
                    const bool held = dbias_held_[i] && g.size() == b.size();
                    all.push_back({ParamKey(which == 0 ? PARAM_EDGE_BIAS_S : PARAM_EDGE_BIAS_ST, (int)i, 0), b.data(), 1, held ? g.data() : nullptr, 1,
                                   (int64_t)b.size(), 1, "Error, GAT optimizer_step needs the edge-bias gradient of a backwardPass since set_edge_bias_learned!"});
                }
            }
            if (norm_[i] != HNH_GAT_NORM_LAYER) continue;
            const DenseMatrix& g = norm_grads_[i];  // (2 x H f: dgamma, then dbeta)
            const bool have = norm_grads_held_[i] && g.rows() == 2 && g.cols() == hf;
            const char* refusal = "Error, GAT optimizer_step needs the norm gradient of a backwardPass since set_norm!";
            all.push_back({ParamKey(PARAM_NORM_GAIN, (int)i, 0), norm_gain_[i].data(), 1, have ? g.data() : nullptr, 1, hf, 1, refusal});
            all.push_back({ParamKey(PARAM_NORM_SHIFT, (int)i, 0), norm_shift_[i].data(), 1, have ? g.data() + hf : nullptr, 1, hf, 1, refusal});
        }
        return all;
    }
    // The moments of a learned tensor, on the compute stream: zeroed when the tensor is first learned after set_optimizer (the bias
    // correction is the global step count's), kept from then on, also while the tensor is switched off.
    const Moments& ensure_moments(const Learned& t) {
        Moments& m = moments_[t.key];
        if (m.second.rows() != t.rows || m.second.cols() != t.cols) {
            if (optim_.kind != HNH_OPTIM_SGD) m.first = DenseMatrix::Constant(t.rows, t.cols, 0.0);
            m.second = DenseMatrix::Constant(t.rows, t.cols, 0.0);
        }
        return m;
    }

    bool learns_vectors() const { return score_ == HNH_GAT_SCORE_ADDITIVE || score_ == HNH_GAT_SCORE_GATV2; }
    void check_layer(int i) const {
        if (i < 0 || i >= (int)layers.size()) throw hnh::Error("Error, GAT layer index " + std::to_string(i) + " out of range: " + std::to_string(layers.size()) + " layers!");
    }
    void check_layer_head(int i, int h) const {
        check_layer(i);
        if (h < 0 || h >= layers[(size_t)i].num_heads)
            throw hnh::Error("Error, GAT head index " + std::to_string(h) + " out of range: layer " + std::to_string(i) + " has " + std::to_string(layers[(size_t)i].num_heads) + " heads!");
    }
    void check_qk(int i, int h, int which) const {
        check_layer_head(i, h);
        if (which != 0 && which != 1) throw hnh::Error("Error, GAT query/key weight selector " + std::to_string(which) + " is neither 0 (query) nor 1 (key)!");
    }
    void ensure_qk_weights(int i) {
        const GATLayer& L = layers[(size_t)i];
        for (auto& all : w_qk_) {
            std::vector<DenseMatrix>& w = all[(size_t)i];
            if (w.size() == (size_t)L.num_heads) continue;
            w.clear();
            for (int h = 0; h < L.num_heads; h++) w.push_back(DenseMatrix::Constant(L.wMats[(size_t)h].rows(), L.wMats[(size_t)h].cols(), 0.0));
        }
    }
    int classes_of(int heads_mode) const {
        const GATLayer& L = layers.back();
        return heads_mode == HNH_GAT_HEADS_MEAN ? L.features_per_head : L.num_heads * L.features_per_head;
    }
    int label_classes() const { return classes_of(label_heads_); }
    // one dense block of whole rows per rank: the output's side, and with `input_too` the side of buffers[0], which is laid out like B
    bool whole_rows(bool input_too) const {
        return !d_ops->r_split && d_ops->aSubmatrices.size() == 1 && d_ops->aSubmatrices[0].leftCol == 0 &&
               (!input_too || (d_ops->bSubmatrices.size() == 1 && d_ops->bSubmatrices[0].leftCol == 0));
    }
    // the labels live with the output's rows
    void check_whole_rows(const char* what) const {
        if (!whole_rows(false))
            throw hnh::Error(std::string("Error, GAT ") + what + " needs one dense block of whole rows per rank, which " + d_ops->algorithm_name + " does not have!");
    }
    // Refuses with the first kernel of the list that the library lacks (Backend::missing_kernel, which knows the kernel's header): `what`
    // are the words after "GAT"; HNH_GAT_KERNEL(name) is an entry of the list.
    void require_kernels(const std::string& what, std::initializer_list<std::pair<const void*, const char*>> need) const {
        for (const auto& n : need)
            if (n.first == nullptr) throw hnh::Error(d_ops->world->be->missing_kernel("GAT " + what, n.second));
    }
    // Refuses a schedule on which a rank's own launches do not see all of a row's nonzeros, or an output row is summed across ranks: all
    // but 15d_fusion2 with c = 1 (15d_fusion1 reduce-scatters over the mesh; c > 1, the 2.5D schedules and the sparse shift reduce across
    // ranks too).  `declined`: after a pass, when the schedule itself returned false, having done nothing.
    void require_own_rows(const std::string& what, bool declined = false) const {
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);
        if (!declined && ds != nullptr && !ds->r_split && ds->fusionApproach == 2 && ds->c == 1) return;
        std::string found = d_ops->algorithm_name;
        if (!declined)
            found = (ds ? "15d_fusion" + std::to_string(ds->fusionApproach) + " (" + found + ")" : found) + " with c = " + std::to_string(d_ops->c) +
                    ": its rows are summed across ranks";
        throw hnh::Error("Error, GAT " + what + " supports 15d_fusion2 with c = 1 only, not " + found);
    }
    // The schedule runs a pass at the MOVING operand's width (what its landing buffers and fetches are sized by), and at the head's f
    // again on every exit.
    struct ScheduleWidth {
        Distributed_Sparse* ops;
        int f;
        ScheduleWidth(Distributed_Sparse* ops, int width, int f) : ops(ops), f(f) { ops->setRValue(width); }
        ~ScheduleWidth() { ops->setRValue(f); }
        ScheduleWidth(const ScheduleWidth&) = delete;
        ScheduleWidth& operator=(const ScheduleWidth&) = delete;
    };
    // What an optimizer step under set_grad_clip or with kind AdamW needs of include/hnh_train_clip.h
    void require_clip_kernels() const {
        if (clip_max_ > 0.0)
            require_kernels("gradient clipping", {HNH_GAT_KERNEL(hnh_grad_sumsq_f64_workspace), HNH_GAT_KERNEL(hnh_grad_sumsq_f64), HNH_GAT_KERNEL(hnh_optim_step_clip_f64)});
        if (optimizer_set_ && optim_.kind == HNH_OPTIM_ADAMW) require_kernels("adamw", {HNH_GAT_KERNEL(hnh_optim_step_clip_f64)});
    }
    // Refuses before anything is launched: labels (and the optimizer) not set, then the kernel group, then the row width.
    void check_train_supported(bool need_optimizer) {
        if (!labels_set_ && !multilabel_) throw hnh::Error("Error, GAT loss / train_step / evaluate need set_labels first!");
        if (need_optimizer && !optimizer_set_) throw hnh::Error("Error, GAT train_step needs set_optimizer first!");
        if (need_optimizer) require_clip_kernels();
        if (multilabel_) {  // the sigmoid head: its own kernel group, and no limit on the row width (no row is staged)
            require_kernels("training", {HNH_GAT_KERNEL(hnh_bce_rows_f64_workspace), HNH_GAT_KERNEL(hnh_bce_rows_f64)});
            if (need_optimizer) require_kernels("training", {HNH_GAT_KERNEL(hnh_optim_step_f64)});
            check_whole_rows("loss");
            return;
        }
        require_kernels("training", {HNH_GAT_KERNEL(hnh_xent_rows_f64_workspace), HNH_GAT_KERNEL(hnh_xent_rows_f64)});
        if (need_optimizer) require_kernels("training", {HNH_GAT_KERNEL(hnh_optim_step_f64)});
        const int64_t width = (int64_t)layers.back().num_heads * layers.back().features_per_head;
        if (width > HNH_XENT_MAX_WIDTH)
            throw hnh::Error("Error, GAT loss supports output rows of at most " + std::to_string(HNH_XENT_MAX_WIDTH) + " values, not " + std::to_string(width) +
                             " (include/hnh_train.h)");
        check_whole_rows("loss");
    }
    // This rank's slice of labels_host_ under `mask` (nullptr: every label >= 0), and the labelled count of the world.  Every rank sees
    // the same host arrays, so a refusal is the same on all of them and happens before the collective.
    LabelSet make_label_set(const uint8_t* mask) {
        const int64_t M = d_ops->M;
        const int classes = label_classes();
        int64_t global = 0;
        for (int64_t r = 0; r < M; r++) {
            if (mask != nullptr && !mask[r]) continue;
            const int32_t l = labels_host_[(size_t)r];
            if (l >= classes)
                throw hnh::Error("Error, GAT label " + std::to_string(l) + " of row " + std::to_string(r) + " is out of range: " + std::to_string(classes) + " classes!");
            if (l >= 0) global++;
        }
        if (global == 0) throw hnh::Error("Error, the GAT label mask selects no labelled row!");
        hnh::World* w = d_ops->world;
        const int64_t rows = buffers.back().rows(), top = d_ops->aSubmatrices[0].topRow;
        std::vector<int32_t> local((size_t)rows, -1);
        double mine = 0.0;
        for (int64_t r = 0; r < rows; r++) {
            const int64_t gr = top + r;
            if (gr >= M || (mask != nullptr && !mask[gr]) || labels_host_[(size_t)gr] < 0) continue;
            local[(size_t)r] = labels_host_[(size_t)gr];
            mine += 1.0;
        }
        LabelSet ls;
        ls.labels = hnh::DeviceArray(w, (size_t)rows * sizeof(int32_t));
        if (rows > 0) w->copy(ls.labels.ptr(), local.data(), (size_t)rows * sizeof(int32_t), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        DenseMatrix cnt(1, 1);
        w->copy(cnt.data(), &mine, sizeof(double), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        w->allreduce_f64(w->world_comm(), cnt.data(), 1, HNH_STREAM_COMPUTE);
        w->copy(&ls.count, cnt.data(), sizeof(double), HNH_COPY_D2H, HNH_STREAM_COMPUTE);
        w->sync(HNH_STREAM_COMPUTE);  // (also: `local` and `mine` have been read)
        if (ls.count != (double)global)
            throw hnh::Error("Error, GAT labels: the ranks' rows hold " + std::to_string((int64_t)ls.count) + " labelled rows, the global arrays " + std::to_string(global) + "!");
        return ls;
    }
    // the loss pass and the all-reduce of its two sums on the compute stream; G == nullptr: no gradient
    // the loss pass and the all-reduce of its two sums on the compute stream; G == nullptr: no gradient
    void loss_enqueue(const LabelSet& ls, DenseMatrix* G) {
        const DenseMatrix& out = buffers.back();
        const GATLayer& L = layers.back();
        const int heads = label_heads_ == HNH_GAT_HEADS_MEAN ? L.num_heads : 1;
        if (loss_result_.size() != 2) loss_result_ = DenseMatrix(2, 1);
        const int64_t need = d_ops->world->be->hnh_xent_rows_f64_workspace(out.rows());
        DenseMatrix& work = scratch(SC_XENT_WORK, need, 1);
        HNH_GAT_CALL(hnh_xent_rows_f64, out.data(), out.cols(), (const int32_t*)ls.labels.ptr(), out.rows(), heads, label_classes(), 1.0 / ls.count,
                     G ? G->data() : nullptr, out.cols(), loss_result_.data(), work.data(), need, HNH_STREAM_COMPUTE);
        sum_over_world(loss_result_);
    }
    std::pair<double, double> loss_read(const LabelSet& ls) {
        hnh::World* w = d_ops->world;
        double r[2] = {0.0, 0.0};
        w->copy(r, loss_result_.data(), sizeof(r), HNH_COPY_D2H, HNH_STREAM_COMPUTE);
        w->sync(HNH_STREAM_COMPUTE);
        // a rank that met a bad label reports (NaN, -count); the sum over the world keeps the NaN, while other ranks' `correct` can lift
        // the second word above 0
        if (!(r[1] >= 0.0) || std::isnan(r[0]))
            throw hnh::Error("Error, GAT loss is not a number: the device met a label outside its classes, or the output holds NaN!");
        return {r[0] / ls.count, r[1] / ls.count};
    }
    // This rank's rows of `mask` (nullptr: every row) as bytes on the device, and the selected row count of the world.  Every rank sees
    // the same host array, so a refusal is the same on all of them and happens before the collective.
    TargetSet make_target_set(const uint8_t* mask) {
        const int64_t M = d_ops->M;
        int64_t global = M;
        if (mask != nullptr) {
            global = 0;
            for (int64_t r = 0; r < M; r++) global += mask[r] ? 1 : 0;
        }
        if (global == 0) throw hnh::Error("Error, the GAT multi-label mask selects no row!");
        hnh::World* w = d_ops->world;
        const int64_t rows = buffers.back().rows(), top = d_ops->aSubmatrices[0].topRow;
        std::vector<uint8_t> local((size_t)rows, 0);
        double mine = 0.0;
        for (int64_t r = 0; r < rows && top + r < M; r++) {
            if (mask != nullptr && !mask[top + r]) continue;
            local[(size_t)r] = 1;
            mine += 1.0;
        }
        TargetSet ts;
        ts.mask = hnh::DeviceArray(w, (size_t)rows);
        if (rows > 0) w->copy(ts.mask.ptr(), local.data(), (size_t)rows, HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        DenseMatrix cnt(1, 1);
        w->copy(cnt.data(), &mine, sizeof(double), HNH_COPY_H2D, HNH_STREAM_COMPUTE);
        w->allreduce_f64(w->world_comm(), cnt.data(), 1, HNH_STREAM_COMPUTE);
        w->copy(&ts.count, cnt.data(), sizeof(double), HNH_COPY_D2H, HNH_STREAM_COMPUTE);
        w->sync(HNH_STREAM_COMPUTE);  // (also: `local` and `mine` have been read)
        if (ts.count != (double)global)
            throw hnh::Error("Error, GAT multi-label targets: the ranks' rows hold " + std::to_string((int64_t)ts.count) + " selected rows, the global mask " +
                             std::to_string(global) + "!");
        return ts;
    }
    // the sigmoid head's loss pass and the all-reduce of its four sums on the compute stream; G == nullptr: no gradient
    void bce_enqueue(const TargetSet& ts, DenseMatrix* G) {
        const DenseMatrix& out = buffers.back();
        const int classes = classes_of(ml_heads_);
        const int heads = ml_heads_ == HNH_GAT_HEADS_MEAN ? layers.back().num_heads : 1;
        if (ml_result_.size() != 4) ml_result_ = DenseMatrix(4, 1);
        const int64_t need = d_ops->world->be->hnh_bce_rows_f64_workspace(out.rows());
        DenseMatrix& work = scratch(SC_BCE_WORK, need, 1);
        HNH_GAT_CALL(hnh_bce_rows_f64, out.data(), out.cols(), (const uint32_t*)ml_bits_.ptr(), ml_words_, (const uint8_t*)ts.mask.ptr(),
                     ml_weights_.size() ? ml_weights_.data() : nullptr, out.rows(), heads, classes, 1.0 / (ts.count * classes), G ? G->data() : nullptr,
                     out.cols(), ml_result_.data(), work.data(), need, HNH_STREAM_COMPUTE);
        sum_over_world(ml_result_);
    }
    // (mean loss over selected rows x classes, micro-F1 = 2 tp / (2 tp + fp + fn), 0 when nothing is predicted or present); keeps the counts
    std::pair<double, double> bce_read(const TargetSet& ts) {
        hnh::World* w = d_ops->world;
        double r[4] = {0.0, 0.0, 0.0, 0.0};
        w->copy(r, ml_result_.data(), sizeof(r), HNH_COPY_D2H, HNH_STREAM_COMPUTE);
        w->sync(HNH_STREAM_COMPUTE);
        if (std::isnan(r[0])) throw hnh::Error("Error, GAT loss is not a number: the output holds NaN!");
        for (int k = 0; k < 3; k++) ml_counts_[k] = r[k + 1];
        const double denom = 2.0 * r[1] + r[2] + r[3];
        return {r[0] / (ts.count * classes_of(ml_heads_)), denom > 0.0 ? 2.0 * r[1] / denom : 0.0};
    }
    DenseMatrix scored[2];  // score ADDITIVE: [A (0) | s t] of the head in flight and of the next one (include/hnh_attn_additive.h)
    // softmax attention: the rows' running max / sum (reused by every head, which run one after the other on the compute stream), the
    // log-sum-exp of every (layer, head), and for the backward pass a column of ones and the broadcasts of lse and delta onto the nonzeros
    DenseMatrix row_max_, row_sum_, ones_col_;
    std::vector<std::vector<DenseMatrix>> lse_;
    VectorXd lse_S_, delta_S_, lse_ST_, delta_ST_;
    VectorXd ones_S_, ones_ST_, e_S_, d_S_, e_ST_, d_ST_;  // backward: S values (= 1) and the recomputed / gated value vectors
    // Work buffers by (role, rows, cols).  A role has one call site, but for two that are shared on purpose: SC_TN_WORK, the split-K
    // workspace of every X^T D product of gemm_tn, and SC_PACKED, the packed P = [A | dZ | lse delta] of the fused and the gatv2 backward.
    enum ScratchRole { SC_DA_ALL, SC_WT, SC_A, SC_DZ, SC_DA_ROW, SC_T1, SC_T2, SC_TN_WORK, SC_DELTA, SC_PACKED, SC_ADD_M, SC_ADD_Q, SC_ADD_D, SC_ADD_DAGG,
                       SC_ADD_TN_WORK, SC_XENT_WORK, SC_V2_R, SC_V2_C, SC_V2_DAGG, SC_V2_WORK, SC_COEF_A, SC_COEF_S, SC_COEF_T, SC_RES_PRODUCT, SC_DZ_ALL,
                       SC_COLSUM_WORK, SC_DX_RES, SC_QKV_Q, SC_QKV_K, SC_QKV_KV, SC_QKV_P, SC_QKV_DQ, SC_QKV_DK, SC_QKV_DX, SC_NORM_G, SC_NORM_WORK, SC_BCE_WORK, SC_SUMSQ_WORK };
    std::map<std::tuple<int, int64_t, int64_t>, DenseMatrix> scratch_;

    // m at rows x cols: allocated anew (on the compute stream) unless it has that shape already
    static DenseMatrix& shaped(DenseMatrix& m, int64_t rows, int64_t cols) {
        if (m.rows() != rows || m.cols() != cols) m = DenseMatrix(rows, cols);
        return m;
    }
    DenseMatrix& scratch_slot(ScratchRole role, int64_t rows, int64_t cols) { return scratch_[std::make_tuple((int)role, rows, cols)]; }  // (not shaped yet)
    DenseMatrix& scratch(ScratchRole role, int64_t rows, int64_t cols) { return shaped(scratch_slot(role, rows, cols), rows, cols); }
    void sum_over_world(double* data, size_t n) {
        hnh::World* w = d_ops->world;
        w->allreduce_f64(w->world_comm(), data, n, HNH_STREAM_COMPUTE);
    }
    void sum_over_world(DenseMatrix& m) { sum_over_world(m.data(), (size_t)m.size()); }
    // C (m x n at pitch ldc) = A^T B over `rows` local rows on the compute stream, the split-K workspace of hnh_gemm_tn_f64 from the scratch
    void gemm_tn(int64_t m, int64_t n, int64_t rows, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, ScratchRole work_role) {
        const int64_t need = d_ops->world->be->hnh_gemm_tn_f64_workspace(m, n, rows);
        double* work = need > 0 ? scratch(work_role, need, 1).data() : nullptr;
        HNH_GAT_CALL(hnh_gemm_tn_f64, m, n, rows, A, lda, B, ldb, C, ldc, work, need, HNH_STREAM_COMPUTE);
    }
    // grad = X^T D over the local rows, then over every rank (the dense rows of the 1.5D layout are not replicated)
    void world_grad_tn(DenseMatrix& grad, const DenseMatrix& X, const DenseMatrix& D) {
        shaped(grad, X.cols(), D.cols());
        gemm_tn(X.cols(), D.cols(), X.rows(), X.data(), X.cols(), D.data(), D.cols(), grad.data(), D.cols(), SC_TN_WORK);
        sum_over_world(grad);
    }

    static uint32_t drop_threshold(double p) { return (uint32_t)std::floor(p * 4294967296.0); }  // keep iff word 0 >= floor(p 2^32)
    // the key of (layer i, head j)'s attention mask on this rank's rows
    hnh_attn_drop attn_drop_args(int i, int j) const {
        hnh_attn_drop d = {};
        d.seed = seed_;
        d.w2 = (uint32_t)i * 65536u + (uint32_t)j;
        d.threshold = drop_threshold(attn_p_);
        d.scale = 1.0 / (1.0 - attn_p_);
        d.row_id0 = d_ops->aSubmatrices[0].topRow;
        return d;
    }
    // the input of layer i as the products and the dW GEMM see it: Xd with feature dropout, the buffer itself without
    DenseMatrix& layer_input(int i) { return feat_p_ > 0.0 ? xd_.at((size_t)i) : buffers[(size_t)i]; }
    // dst = c_q mask o src with layer i's feature mask (dst == src allowed), on the compute stream
    void feature_mask(int i, DenseMatrix& dst, const DenseMatrix& src) {
        const DenseSubmatrix& sub = i == 0 ? d_ops->bSubmatrices[0] : d_ops->aSubmatrices[0];  // (buffers[0] is laid out like B)
        HNH_GAT_CALL(hnh_feat_drop_f64, dst.data(), dst.cols(), src.data(), src.cols(), src.rows(), src.cols(), sub.topRow, seed_, (uint32_t)i,
                     drop_threshold(feat_p_), 1.0 / (1.0 - feat_p_), HNH_STREAM_COMPUTE);
    }
    void drop_input(int i) {
        if (!(feat_p_ > 0.0)) return;
        if (xd_.size() != buffers.size() - 1) xd_.assign(buffers.size() - 1, DenseMatrix());
        DenseMatrix& X = buffers[(size_t)i];
        feature_mask(i, shaped(xd_[(size_t)i], X.rows(), X.cols()), X);
    }

    // Dropout's own conditions, checked before anything is launched (and before the additive score's, whose kernel group a library
    // may lack as well): the score, the counter's field widths, the layout, then its kernel group.
    void check_dropout_supported() {
        if (!(attn_p_ > 0.0) && !(feat_p_ > 0.0)) return;
        if (attn_p_ > 0.0 && score_ != HNH_GAT_SCORE_ADDITIVE)
            throw hnh::Error(std::string("Error, GAT attention dropout supports score additive only, not score ") +
                             (score_ == HNH_GAT_SCORE_GATV2         ? "gatv2: the gatv2 passes have no mask "
                              : score_ == HNH_GAT_SCORE_TRANSFORMER ? "transformer: the query/key/value passes have no mask "
                                                                    : "dot: the dot-product passes have no mask ") +
                             "(include/hnh_attn_dropout.h)");
        if (d_ops->M > 4294967296LL || d_ops->N > 4294967296LL || layers.size() > 65536)
            throw hnh::Error("Error, GAT dropout needs row ids below 2^32 and at most 65536 layers (the generator's counter words)!");
        for (const GATLayer& L : layers)
            if (L.num_heads > 65536 || (int64_t)L.input_features > 4294967296LL)
                throw hnh::Error("Error, GAT dropout needs at most 65536 heads per layer (the generator's counter words)!");
        if (feat_p_ > 0.0 && !whole_rows(true))
            throw hnh::Error("Error, GAT feature dropout needs one dense block of whole rows per rank, which " + d_ops->algorithm_name + " does not have!");
        if (attn_p_ > 0.0)
            require_kernels("dropout", {HNH_GAT_KERNEL(hnh_attn_drop_fwd_csr_p), HNH_GAT_KERNEL(hnh_attn_drop_row_csr_p), HNH_GAT_KERNEL(hnh_attn_drop_col_csr_p),
                             HNH_GAT_KERNEL(hnh_attn_drop_scores_f64), HNH_GAT_KERNEL(hnh_attn_drop_pack_f64)});
        if (feat_p_ > 0.0) require_kernels("dropout", {HNH_GAT_KERNEL(hnh_feat_drop_f64)});
    }

    static const char* activation_name(int mode) { return mode == HNH_GAT_ACT_ELU ? "elu" : (mode == HNH_GAT_ACT_IDENTITY ? "identity" : "relu"); }
    // the finishing call's flag of layer i's activation (include/hnh_attention.h); 0 for relu; identity for a normalised layer, whose
    // activation follows the normalisation
    unsigned activation_flag(int i) const {
        const int m = head_act(i);
        return m == HNH_GAT_ACT_ELU ? HNH_ATTN_ACT_ELU : (m == HNH_GAT_ACT_IDENTITY ? HNH_ATTN_ACT_IDENTITY : 0u);
    }
    // ---- layer normalisation (include/hnh_gat_norm.h)
    bool normed(int i) const { return norm_[(size_t)i] == HNH_GAT_NORM_LAYER; }
    // where the heads of layer i write and what the backward pass reads as the layer's stored output: the pre-normalisation rows of a
    // normalised layer, the layer's output buffer otherwise; and the activation those rows went through: none for a normalised layer
    DenseMatrix& head_target(int i) { return normed(i) ? pre_[(size_t)i] : buffers[(size_t)i + 1]; }
    int head_act(int i) const { return normed(i) ? HNH_GAT_ACT_IDENTITY : act_[(size_t)i]; }
    void ensure_norm_weights(int i) {
        const int64_t hf = (int64_t)layers[(size_t)i].num_heads * layers[(size_t)i].features_per_head;
        if (norm_gain_[(size_t)i].rows() != hf) norm_gain_[(size_t)i] = DenseMatrix::Constant(hf, 1, 1.0);
        if (norm_shift_[(size_t)i].rows() != hf) norm_shift_[(size_t)i] = DenseMatrix::Constant(hf, 1, 0.0);
    }
    void check_norm_vectors(int i, const double* a, const double* b, int64_t n, const char* who) const {
        check_layer(i);
        if (a == nullptr || b == nullptr) throw hnh::Error(std::string("Error, GAT ") + who + ": null pointer!");
        const int64_t hf = (int64_t)layers[(size_t)i].num_heads * layers[(size_t)i].features_per_head;
        if (n != hf)
            throw hnh::Error(std::string("Error, GAT ") + who + " of layer " + std::to_string(i) + " needs gamma and beta of num_heads * features_per_head = " +
                             std::to_string(hf) + " entries each, not " + std::to_string(n) + "!");
    }
    // pre_[i] and the stats of a normalised layer, on the compute stream (before the layer's ev_input mark)
    void shape_pre(int i) {
        if (!normed(i)) return;
        const DenseMatrix& out = buffers[(size_t)i + 1];
        shaped(pre_[(size_t)i], out.rows(), out.cols());
        shaped(norm_stats_[(size_t)i], out.rows(), 2);
    }
    // buffers[i + 1] = phi_i(gamma o xh + beta) from pre_[i], on the compute stream behind the layer's last head; nothing for a layer without
    void norm_forward(int i) {
        if (!normed(i)) return;
        DenseMatrix &out = buffers[(size_t)i + 1], &z = pre_[(size_t)i];
        HNH_GAT_CALL(hnh_layernorm_fwd_f64, out.data(), out.cols(), z.data(), z.cols(), norm_stats_[(size_t)i].data(), norm_gain_[(size_t)i].data(),
                     norm_shift_[(size_t)i].data(), z.rows(), z.cols(), norm_eps_[(size_t)i], kernel_activation(act_[(size_t)i]), HNH_STREAM_COMPUTE);
    }
    // G' = dL/d(pre_[i]) from G = dL/d(buffers[i + 1]) into its scratch, and norm_grads_[i] = [dgamma; dbeta] summed over the world
    const DenseMatrix& norm_backward(int i, const DenseMatrix& G) {
        const int S0 = HNH_STREAM_COMPUTE;
        const DenseMatrix& z = pre_[(size_t)i];
        const int64_t rows = z.rows(), hf = z.cols();
        if (G.rows() != rows || G.cols() != hf || norm_stats_[(size_t)i].rows() != rows)
            throw hnh::Error("Error, GAT backwardPass: the normalised layer's stored rows do not have the layer's shape!");
        DenseMatrix& Gp = scratch(SC_NORM_G, rows, hf);
        DenseMatrix& dgb = shaped(norm_grads_[(size_t)i], 2, hf);
        const int64_t need = d_ops->world->be->hnh_layernorm_bwd_workspace(rows, hf);
        double* work = need > 0 ? scratch(SC_NORM_WORK, need, 1).data() : nullptr;
        HNH_GAT_CALL(hnh_layernorm_bwd_f64, Gp.data(), hf, dgb.data(), dgb.data() + hf, G.data(), hf, z.data(), hf, norm_stats_[(size_t)i].data(),
                     norm_gain_[(size_t)i].data(), norm_shift_[(size_t)i].data(), rows, hf, kernel_activation(act_[(size_t)i]), work, need, S0);
        sum_over_world(dgb);
        norm_grads_held_[(size_t)i] = 1;
        return Gp;
    }

    // ---- bias and skip connections (include/hnh_gat_skip.h)
    bool has_addend(int i) const { return bias_on_[(size_t)i] != 0 || res_mode_[(size_t)i] != HNH_GAT_RESIDUAL_NONE; }
    // the finishing call's HNH_ATTN_ADDEND of a layer whose heads have an addend; 0 without: today's launches
    unsigned addend_flag(int i) const { return has_addend(i) ? HNH_ATTN_ADDEND : 0u; }
    void ensure_residual_weight(int i) {
        GATLayer& L = layers[(size_t)i];
        std::vector<DenseMatrix>& wr = w_res_[(size_t)i];
        if (wr.size() == (size_t)L.num_heads) return;
        wr.clear();
        for (int h = 0; h < L.num_heads; h++) wr.push_back(DenseMatrix::Constant(L.wMats[(size_t)h].rows(), L.wMats[(size_t)h].cols(), 0.0));
    }
    // W_res of layer i between one HOST matrix and the per-head operands: from `src` to the device, or from the device into `dst`
    void copy_residual_weight(int i, const double* src, double* dst) {
        const GATLayer& L = layers[(size_t)i];
        const int64_t k = L.input_features, f = L.features_per_head, hf = (int64_t)L.num_heads * f;
        std::vector<double> head((size_t)(k * f));
        for (int h = 0; h < L.num_heads; h++) {
            DenseMatrix& Wr = w_res_[(size_t)i][(size_t)h];
            if (dst && Wr.size()) Wr.copy_to_host(head.data());
            for (int64_t r = 0; r < k; r++) {
                const int64_t at = r * hf + (int64_t)h * f;
                if (dst) std::memcpy(dst + at, head.data() + r * f, sizeof(double) * (size_t)f);
                else std::memcpy(head.data() + r * f, src + at, sizeof(double) * (size_t)f);
            }
            if (src) Wr.copy_from_host(head.data());  // (waits for the copy: `head` is reused)
        }
    }
    // head h's slice of layer i's a1 (q = 0) or a2 (q = 1), after ensure_attn_vectors
    double* attn_vector(int i, int h, int q) {
        GATLayer& L = layers[(size_t)i];
        return (q == 0 ? L.a1 : L.a2).data() + (int64_t)h * L.features_per_head;
    }
    // both slices of (layer i, head h) from the host (HNH_COPY_H2D) or to it (HNH_COPY_D2H) on the compute stream, waited for
    void copy_attn_vectors(int i, int h, double* a1_host, double* a2_host, int kind) {
        hnh::World* w = d_ops->world;
        double* host[2] = {a1_host, a2_host};
        const size_t bytes = (size_t)layers[(size_t)i].features_per_head * sizeof(double);
        for (int q = 0; q < 2; q++) {
            double* dev = attn_vector(i, h, q);
            w->copy(kind == HNH_COPY_H2D ? dev : host[q], kind == HNH_COPY_H2D ? host[q] : dev, bytes, kind, HNH_STREAM_COMPUTE);
        }
        w->sync(HNH_STREAM_COMPUTE);
    }
    static const char* residual_name(int mode) { return mode == HNH_GAT_RESIDUAL_IDENTITY ? "identity" : (mode == HNH_GAT_RESIDUAL_PROJECTION ? "projection" : "none"); }
    // the auxiliary stream's scratch for X W_res_h (allocated before the layer's ev_input mark, like the product buffers)
    void shape_residual(int i) {
        if (res_mode_[(size_t)i] == HNH_GAT_RESIDUAL_PROJECTION) shaped(res_product_, buffers[(size_t)i].rows(), layers[(size_t)i].features_per_head);
    }
    // The residual r of (layer i, head h) as the skip kernels take it: none, the head's column block of X (identity), or X W_res_h computed
    // on `stream` into `buffer` (projection; shaped here if it is not yet).  No addend is kept between the passes: the forward pass computes
    // the product on the stream of the head's product stage into res_product_, the backward pass again on the compute stream into its scratch.
    struct Operand {
        const double* data;
        int64_t ld;
    };
    Operand residual_operand(int i, int h, int stream, DenseMatrix& buffer) {
        DenseMatrix& X = layer_input(i);
        const int64_t f = layers[(size_t)i].features_per_head;
        if (res_mode_[(size_t)i] == HNH_GAT_RESIDUAL_IDENTITY) return {X.data() + (int64_t)h * f, X.cols()};
        if (res_mode_[(size_t)i] != HNH_GAT_RESIDUAL_PROJECTION) return {nullptr, 0};
        shaped(buffer, X.rows(), f);
        HNH_GAT_CALL(hnh_gemm_f64, X.rows(), f, X.cols(), X.data(), w_res_[(size_t)i].at((size_t)h).data(), buffer.data(), stream);
        return {buffer.data(), f};
    }
    const double* head_bias(int i, int h) const {
        return bias_on_[(size_t)i] ? bias_[(size_t)i].data() + (int64_t)h * layers[(size_t)i].features_per_head : nullptr;
    }
    // the addend r + b of (layer i, head j) into the head's column block of buffers[i + 1] (pre_[i] of a normalised layer), on `stream`;
    // nothing for a layer without
    void head_addend(int i, int j, int stream) {
        if (!has_addend(i)) return;
        DenseMatrix& out = head_target(i);
        const int64_t f = layers[(size_t)i].features_per_head;
        const Operand res = residual_operand(i, j, stream, res_product_);
        HNH_GAT_CALL(hnh_skip_addend_cols_f64, out.data(), out.cols(), (int64_t)j * f, res.data, res.ld, head_bias(i, j), out.rows(), f, stream);
    }

    // ---- support.  Four conditions recur in the optional features' checks: attention softmax (require_softmax), a schedule on which a rank's
    // own launches see whole rows (require_own_rows), a head width (require_head_width) and a kernel group (require_kernels).  Each feature's
    // check below runs its conditions in its own order, and check_supported runs the features' checks in the entry point's order; every
    // refusal happens before anything is launched.
    void require_softmax(const std::string& what, const char* why, const char* header) const {
        if (attention_ != HNH_GAT_ATTENTION_SOFTMAX)
            throw hnh::Error("Error, GAT " + what + " supports attention mode softmax only, not attention mode none" + why + " (" + header + ")");
    }
    // heads of at most `limit` features on layer `only`, or on every layer
    void require_head_width(const std::string& what, int limit, const char* header, int only = -1) const {
        for (size_t i = 0; i < layers.size(); i++)
            if ((only < 0 || (int)i == only) && layers[i].features_per_head > limit)
                throw hnh::Error("Error, GAT " + what + " supports heads of at most " + std::to_string(limit) + " features, not " +
                                 std::to_string(layers[i].features_per_head) + " (" + header + ")");
    }
    // A layer with a bias or a skip connection: the finish of a softmax pass takes the addend; the shapes of residual identity.
    void check_skip_supported() {
        for (size_t i = 0; i < layers.size(); i++) {
            if (!has_addend((int)i)) continue;
            const std::string what = (res_mode_[i] != HNH_GAT_RESIDUAL_NONE ? std::string("residual ") + residual_name(res_mode_[i]) : std::string("bias")) +
                                     " of layer " + std::to_string(i);
            require_softmax(what, ": its passes have no addend", "include/hnh_gat_skip.h");
            require_own_rows(what);
            if (res_mode_[i] == HNH_GAT_RESIDUAL_IDENTITY) {
                const DenseMatrix &X = buffers[i], &out = buffers[i + 1];
                // (layer 0's input is laid out like B: its local row r must be the output's local row r)
                const bool same_rows = i > 0 || (whole_rows(true) && d_ops->bSubmatrices[0].topRow == d_ops->aSubmatrices[0].topRow);
                if (layers[i].input_features != layers[i].num_heads * layers[i].features_per_head || X.rows() != out.rows() || X.cols() != out.cols() || !same_rows)
                    throw hnh::Error("Error, GAT " + what + " needs an input and an output of the same shape, not " + std::to_string(X.rows()) + " x " +
                                     std::to_string(X.cols()) + " and " + std::to_string(out.rows()) + " x " + std::to_string(out.cols()) +
                                     ": use residual projection!");
            }
            require_kernels(what, {HNH_GAT_KERNEL(hnh_skip_addend_cols_f64), HNH_GAT_KERNEL(hnh_skip_grad_cols_f64), HNH_GAT_KERNEL(hnh_colsum_f64_workspace),
                             HNH_GAT_KERNEL(hnh_colsum_f64)});
        }
    }
    // A non-ReLU layer: attention none ends in the fused pair's or the un-fused route's ReLU; a kernel library that knows the activation
    // flags is one that exports hnh_act_grad_cols_f64.
    void check_activation_supported() {
        for (size_t i = 0; i < layers.size(); i++) {
            if (act_[i] == HNH_GAT_ACT_RELU) continue;
            const std::string what = std::string("activation ") + activation_name(act_[i]) + " of layer " + std::to_string(i);
            require_softmax(what, ": its passes end in a ReLU", "include/hnh_attention.h");
            require_own_rows(what);
            require_kernels(what, {HNH_GAT_KERNEL(hnh_act_grad_cols_f64)});
        }
    }
    // A normalised layer: its heads end in the identity flag of the softmax passes' finishing launch and its backward pass in
    // hnh_act_grad_cols_f64's identity, so it is supported where the activations are; the row width; its kernel group.
    void check_norm_supported() {
        for (size_t i = 0; i < layers.size(); i++) {
            if (!normed((int)i)) continue;
            const std::string what = "norm layer of layer " + std::to_string(i);
            require_softmax(what, ": its passes end in a ReLU", "include/hnh_gat_norm.h");
            require_own_rows(what);
            const int64_t hf = (int64_t)layers[i].num_heads * layers[i].features_per_head;
            if (hf > HNH_NORM_MAX_COLS)
                throw hnh::Error("Error, GAT " + what + " supports rows of at most " + std::to_string(HNH_NORM_MAX_COLS) + " values (num_heads * features_per_head), not " +
                                 std::to_string(hf) + " (include/hnh_gat_norm.h)");
            require_kernels(what, {HNH_GAT_KERNEL(hnh_layernorm_fwd_f64), HNH_GAT_KERNEL(hnh_layernorm_bwd_workspace), HNH_GAT_KERNEL(hnh_layernorm_bwd_f64)});
            require_kernels(what, {HNH_GAT_KERNEL(hnh_act_grad_cols_f64)});
        }
    }
    // The backward pass: the score's or the fused mode's own conditions first, then the plain pass's schedules and kernel groups.
    void check_backward_supported() {
        if (score_ == HNH_GAT_SCORE_ADDITIVE) check_additive_supported();
        else if (score_ == HNH_GAT_SCORE_GATV2) check_gatv2_supported();
        else if (score_ == HNH_GAT_SCORE_TRANSFORMER) check_transformer_supported();
        else if (backward_ == HNH_GAT_BACKWARD_FUSED) check_fused_backward_supported();
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);
        if (ds == nullptr || ds->r_split)
            throw hnh::Error("Error, GAT backwardPass supports the 1.5D dense-shift schedules only (15d_fusion1, 15d_fusion2 with c = 1), not " +
                             d_ops->algorithm_name);
        if (ds->fusionApproach == 2 && ds->c != 1)
            throw hnh::Error("Error, GAT backwardPass does not support 15d_fusion2 with c > 1 (its forward pass reproduces a quirk of the reference)");
        require_kernels("backwardPass", {HNH_GAT_KERNEL(hnh_gemm_tn_f64_workspace), HNH_GAT_KERNEL(hnh_gemm_tn_f64), HNH_GAT_KERNEL(hnh_leaky_relu_grad_f64),
                         HNH_GAT_KERNEL(hnh_relu_grad_cols_f64), HNH_GAT_KERNEL(hnh_sum3_cols_f64), HNH_GAT_KERNEL(hnh_transpose_into_f64)});
        if (attention_ == HNH_GAT_ATTENTION_SOFTMAX)
            require_kernels("backwardPass with softmax attention", {HNH_GAT_KERNEL(hnh_softmax_gate_f64), HNH_GAT_KERNEL(hnh_rowdot_cols_f64)});
    }
    // The fused backward mode: its kernel group first.
    void check_fused_backward_supported() {
        require_kernels("backwardPass in fused mode", {HNH_GAT_KERNEL(hnh_attn_grad_row_csr_p), HNH_GAT_KERNEL(hnh_attn_grad_col_csr_p), HNH_GAT_KERNEL(hnh_attn_grad_pack_f64)});
        require_own_rows("fused backward");
        require_head_width("fused backward", HNH_ATTN_GRAD_MAX_F, "include/hnh_attn_grad.h");
    }
    void check_additive_supported() {
        require_softmax("score additive", "", "include/hnh_attn_additive.h");
        require_own_rows("score additive");
        require_head_width("score additive", HNH_ATTN_ADD_MAX_F, "include/hnh_attn_additive.h");
        require_kernels("score additive", {HNH_GAT_KERNEL(hnh_attn_add_fwd_csr_p), HNH_GAT_KERNEL(hnh_attn_add_row_csr_p), HNH_GAT_KERNEL(hnh_attn_add_col_csr_p),
                         HNH_GAT_KERNEL(hnh_attn_add_scores_f64), HNH_GAT_KERNEL(hnh_attn_add_pack_f64), HNH_GAT_KERNEL(hnh_attn_add_update_f64)});
    }
    // The gatv2 score: no attention dropout (its passes have no mask); its kernel group and the pack kernel of the fused backward it reuses.
    void check_gatv2_supported() {
        require_softmax("score gatv2", "", "include/hnh_attn_v2.h");
        require_own_rows("score gatv2");
        require_head_width("score gatv2", HNH_ATTN_V2_MAX_F, "include/hnh_attn_v2.h");
        if (attn_p_ > 0.0)
            throw hnh::Error("Error, GAT score gatv2 does not support attention dropout (p = " + std::to_string(attn_p_) +
                             "): its passes have no mask (include/hnh_attn_v2.h)");
        require_kernels("score gatv2", {HNH_GAT_KERNEL(hnh_attn_v2_fwd_csr_p), HNH_GAT_KERNEL(hnh_attn_v2_row_csr_p), HNH_GAT_KERNEL(hnh_attn_v2_col_csr_p),
                         HNH_GAT_KERNEL(hnh_attn_v2_finish_f64)});
        require_kernels("score gatv2", {HNH_GAT_KERNEL(hnh_attn_grad_pack_f64)});
    }
    // The transformer score: no attention dropout (its passes have no mask); its kernel group and the pack kernel of the fused backward,
    // which builds all of its gathered operands.
    void check_transformer_supported() {
        require_softmax("score transformer", "", "include/hnh_attn_qkv.h");
        require_own_rows("score transformer");
        require_head_width("score transformer", HNH_ATTN_QKV_MAX_F, "include/hnh_attn_qkv.h");
        if (attn_p_ > 0.0)
            throw hnh::Error("Error, GAT score transformer does not support attention dropout (p = " + std::to_string(attn_p_) +
                             "): its passes have no mask (include/hnh_attn_qkv.h)");
        require_kernels("score transformer", {HNH_GAT_KERNEL(hnh_attn_qkv_fwd_csr_p), HNH_GAT_KERNEL(hnh_attn_qkv_row_csr_p), HNH_GAT_KERNEL(hnh_attn_qkv_col_csr_p)});
        require_kernels("score transformer", {HNH_GAT_KERNEL(hnh_attn_grad_pack_f64)});
    }
    // A layer with an edge bias: the transformer score's passes alone take one (its own conditions are check_transformer_supported's, which
    // follows); the kernel group.
    // A layer whose bias is learned needs the gradient's group as well wherever a backward pass runs, asked for first: it is what the
    // layer's backward pass launches.
    void check_edge_bias_supported(bool backward) {
        for (size_t i = 0; i < layers.size(); i++) {
            if (!edge_bias_on_[i]) continue;
            const std::string what = "edge bias of layer " + std::to_string(i);
            if (score_ != HNH_GAT_SCORE_TRANSFORMER)
                throw hnh::Error("Error, GAT " + what + " supports score transformer only, not score " + score_name(score_) +
                                 ": its passes have no bias operand (include/hnh_attn_edge.h)");
            if (backward && edge_bias_learned_[i])
                require_kernels("learned edge bias", {HNH_GAT_KERNEL(hnh_attn_qkv_bias_grad_row_csr_p), HNH_GAT_KERNEL(hnh_attn_qkv_bias_grad_col_csr_p)});
            require_kernels("edge bias", {HNH_GAT_KERNEL(hnh_attn_qkv_bias_fwd_csr_p), HNH_GAT_KERNEL(hnh_attn_qkv_bias_row_csr_p),
                             HNH_GAT_KERNEL(hnh_attn_qkv_bias_col_csr_p)});
        }
    }
    static const char* score_name(int score) {
        return score == HNH_GAT_SCORE_DOT ? "dot" : score == HNH_GAT_SCORE_ADDITIVE ? "additive" : score == HNH_GAT_SCORE_GATV2 ? "gatv2" : "transformer";
    }
    // Softmax attention with score dot: a row's softmax needs all of the row's nonzeros summed by this rank's own launches.
    void check_softmax_supported() {
        require_own_rows("softmax attention");
        // a head is one pass over its columns (include/hnh_attention.h); its operands are whole allocations and column blocks at an even
        // offset of an even pitch when f is even, so the 16-byte condition of the 512 limit holds for every even f
        for (const GATLayer& L : layers) {
            const int f = L.features_per_head;
            if (f > 512 || (f % 2 != 0 && f > 256))
                throw hnh::Error("Error, GAT softmax attention supports heads of at most 512 features (256 when odd), not " + std::to_string(f) +
                                 ": a row's softmax is one pass over its columns (include/hnh_attention.h)");
        }
        require_kernels("softmax attention", {HNH_GAT_KERNEL(hnh_attn_softmax_csr_p)});
    }
    // What an entry point refuses, in one order: the training state (labels, optimizer, training kernels, output width, whole rows), then
    // dropout, the activations, the norms, bias and skip connections, the edge bias, then the backward pass's conditions or, for a forward pass, the score's own.  The
    // stored forward pass and the shapes of the arguments are the entry point's own checks, afterwards.
    enum Op { OP_FORWARD, OP_BACKWARD, OP_TRAIN_STEP, OP_EVALUATE, OP_LOSS };
    void check_supported(Op op) {
        if (op == OP_TRAIN_STEP || op == OP_EVALUATE || op == OP_LOSS) check_train_supported(op == OP_TRAIN_STEP);
        if (op == OP_LOSS) return;
        check_dropout_supported();
        check_activation_supported();
        check_norm_supported();
        check_skip_supported();
        check_edge_bias_supported(op == OP_BACKWARD || op == OP_TRAIN_STEP);
        if (op == OP_BACKWARD || op == OP_TRAIN_STEP) check_backward_supported();
        if (op != OP_FORWARD) return;  // (evaluate's forwardPass checks the score)
        if (score_ == HNH_GAT_SCORE_ADDITIVE) check_additive_supported();
        else if (score_ == HNH_GAT_SCORE_GATV2) check_gatv2_supported();
        else if (score_ == HNH_GAT_SCORE_TRANSFORMER) check_transformer_supported();
        else if (attention_ == HNH_GAT_ATTENTION_SOFTMAX) check_softmax_supported();
    }

    // the kernels' HNH_ACT_* (include/hnh_grad.h) of a layer's HNH_GAT_ACT_*
    static int kernel_activation(int mode) { return mode == HNH_GAT_ACT_ELU ? HNH_ACT_ELU : (mode == HNH_GAT_ACT_IDENTITY ? HNH_ACT_IDENTITY : HNH_ACT_RELU); }
    // dZ of (layer i, head h) from G and the stored output, on the compute stream.  A plain ReLU layer: hnh_relu_grad_cols_f64 (head_delta
    // computes the delta where a softmax needs one).  Another activation: one launch makes dZ and delta, which waits in act_delta_ for
    // head_delta.  A layer with an addend: the same with the addend taken out of the recovered pre-activation (include/hnh_gat_skip.h), ReLU
    // included, and dZ also into the head's column block of dZ_all.
    void head_dz(int i, int h, const DenseMatrix& G, DenseMatrix& dZ, DenseMatrix* dZ_all) {
        const int S0 = HNH_STREAM_COMPUTE;
        const DenseMatrix& out = head_target(i);  // (a normalised layer: G is dL/d(pre_[i]) and the activation is the identity)
        const int64_t rows = dZ.rows(), f = dZ.cols(), hf = out.cols(), at = (int64_t)h * f;
        const int act = head_act(i);
        if (dZ_all != nullptr) {
            const Operand res = residual_operand(i, h, S0, scratch_slot(SC_RES_PRODUCT, rows, f));
            shaped(act_delta_, rows, 1);
            HNH_GAT_CALL(hnh_skip_grad_cols_f64, dZ.data(), f, dZ_all->data(), hf, act_delta_.data(), G.data(), hf, out.data(), hf, at, res.data, res.ld,
                         head_bias(i, h), rows, f, kernel_activation(act), S0);
        } else if (act == HNH_GAT_ACT_RELU) {
            HNH_GAT_CALL(hnh_relu_grad_cols_f64, dZ.data(), f, G.data(), hf, out.data(), hf, at, rows, f, S0);
        } else {
            shaped(act_delta_, rows, 1);
            HNH_GAT_CALL(hnh_act_grad_cols_f64, dZ.data(), f, act_delta_.data(), G.data(), hf, out.data(), hf, at, rows, f, kernel_activation(act), S0);
        }
    }
    // one layer of the backward pass: G = dL/d(buffers[i + 1]) -> weight_grads[i], input_grads[i]
    void backward_layer(int i, const DenseMatrix& G_out) {
        const int S0 = HNH_STREAM_COMPUTE;
        DenseMatrix& X = layer_input(i);  // (Xd with feature dropout: the forward pass's products used it)
        const DenseMatrix& out = head_target(i);
        // a normalised layer: everything below differentiates the pre-normalisation rows, from G' = dL/d(pre_[i])
        const DenseMatrix& G = normed(i) ? norm_backward(i, G_out) : G_out;
        const int H = layers[(size_t)i].num_heads, f = layers[(size_t)i].features_per_head;
        const int64_t rows = X.rows(), k = X.cols(), hf = (int64_t)H * f;
        if (out.rows() != rows || out.cols() != hf || G.rows() != rows || G.cols() != hf)
            throw hnh::Error("Error, GAT backwardPass: layer buffers do not have the layer's shape!");
        DenseMatrix& dA_all = scratch(SC_DA_ALL, rows, hf);
        DenseMatrix& Wt = scratch(SC_WT, hf, k);
        if (learns_vectors() && score_ == HNH_GAT_SCORE_GATV2) shaped(attn_grads[(size_t)i], hf, 2).setZero();  // (column 1 stays zero; column 0 is written head by head)
        else if (learns_vectors()) shaped(attn_grads[(size_t)i], hf, 2);
        DenseMatrix* dZ_all = has_addend(i) ? &scratch(SC_DZ_ALL, rows, hf) : nullptr;
        const bool qkv = score_ == HNH_GAT_SCORE_TRANSFORMER;
        DenseMatrix* dQ_all = qkv ? &scratch(SC_QKV_DQ, rows, hf) : nullptr;
        DenseMatrix* dK_all = qkv ? &scratch(SC_QKV_DK, rows, hf) : nullptr;
        d_ops->setRValue(f);
        for (int h = 0; h < H; h++) {
            DenseMatrix& Wh = layers[(size_t)i].wMats[(size_t)h];
            DenseMatrix& A = scratch(SC_A, rows, f);
            DenseMatrix& dZ = scratch(SC_DZ, rows, f);
            HNH_GAT_CALL(hnh_gemm_f64, rows, f, k, X.data(), Wh.data(), A.data(), S0);
            head_dz(i, h, G, dZ, dZ_all);
            if (score_ == HNH_GAT_SCORE_ADDITIVE) backward_head_additive(i, h, A, dZ, dA_all);
            else if (score_ == HNH_GAT_SCORE_GATV2) backward_head_gatv2(i, h, A, dZ, dA_all);
            else if (qkv) backward_head_transformer(i, h, A, dZ, dA_all, *dQ_all, *dK_all);
            else if (backward_ == HNH_GAT_BACKWARD_FUSED) backward_head_fused(i, h, A, dZ, dA_all);
            else backward_head_unfused(i, h, A, dZ, dA_all);
            HNH_GAT_CALL(hnh_transpose_into_f64, Wt.data(), k, (int64_t)h * f, Wh.data(), k, f, S0);
        }
        world_grad_tn(weight_grads[(size_t)i], X, dA_all);  // dW_all = X^T dA_all
        if (learns_vectors()) sum_over_world(attn_grads[(size_t)i]);
        // dX = dA_all [W_1^T; ..; W_H^T]
        DenseMatrix& dX = shaped(input_grads[(size_t)i], rows, k);
        HNH_GAT_CALL(hnh_gemm_f64, rows, k, hf, dA_all.data(), Wt.data(), dX.data(), S0);
        if (qkv) {  // dW_q = X^T dQ_all, dW_k = X^T dK_all; dX += dQ_all W_q^T, then dK_all W_k^T (Wt, free by now, takes the transposes)
            DenseMatrix* side[2] = {dQ_all, dK_all};
            DenseMatrix& dXs = scratch(SC_QKV_DX, rows, k);
            for (int which = 0; which < 2; which++) {
                world_grad_tn(qk_weight_grads[which][(size_t)i], X, *side[which]);
                for (int h = 0; h < H; h++)
                    HNH_GAT_CALL(hnh_transpose_into_f64, Wt.data(), k, (int64_t)h * f, w_qk_[which][(size_t)i].at((size_t)h).data(), k, f, S0);
                HNH_GAT_CALL(hnh_gemm_f64, rows, k, hf, side[which]->data(), Wt.data(), dXs.data(), S0);
                HNH_GAT_CALL(hnh_axpy_f64, dX.data(), dXs.data(), 1.0, dX.size(), S0);
            }
        }
        if (dZ_all != nullptr) backward_skip(i, X, *dZ_all, Wt, dX);
        if (feat_p_ > 0.0) feature_mask(i, dX, dX);  // dL/dX = c_q mask o dL/dXd
    }
    // The bias's and the skip connection's share of layer i's backward pass, after the head loop, on the compute stream: db = colsum(dZ_all)
    // and dW_res = X^T dZ_all, both summed over the world like dW, and dX += dZ_all W_res^T (projection; Wt, free by now, takes W_res^T) or
    // dZ_all (identity)
    void backward_skip(int i, DenseMatrix& X, DenseMatrix& dZ_all, DenseMatrix& Wt, DenseMatrix& dX) {
        const int S0 = HNH_STREAM_COMPUTE;
        const int H = layers[(size_t)i].num_heads, f = layers[(size_t)i].features_per_head;
        const int64_t rows = X.rows(), k = X.cols(), hf = (int64_t)H * f;
        if (bias_on_[(size_t)i]) {
            DenseMatrix& db = shaped(bias_grads[(size_t)i], hf, 1);
            const int64_t need = d_ops->world->be->hnh_colsum_f64_workspace(rows, hf);
            double* work = need > 0 ? scratch(SC_COLSUM_WORK, need, 1).data() : nullptr;
            HNH_GAT_CALL(hnh_colsum_f64, db.data(), dZ_all.data(), hf, rows, hf, work, need, S0);
            sum_over_world(db);
        }
        if (res_mode_[(size_t)i] == HNH_GAT_RESIDUAL_PROJECTION) {
            world_grad_tn(res_weight_grads[(size_t)i], X, dZ_all);
            for (int h = 0; h < H; h++)
                HNH_GAT_CALL(hnh_transpose_into_f64, Wt.data(), k, (int64_t)h * f, w_res_[(size_t)i].at((size_t)h).data(), k, f, S0);
            DenseMatrix& dXr = scratch(SC_DX_RES, rows, k);
            HNH_GAT_CALL(hnh_gemm_f64, rows, k, hf, dZ_all.data(), Wt.data(), dXr.data(), S0);
            HNH_GAT_CALL(hnh_axpy_f64, dX.data(), dXr.data(), 1.0, dX.size(), S0);
        } else if (res_mode_[(size_t)i] == HNH_GAT_RESIDUAL_IDENTITY) {
            HNH_GAT_CALL(hnh_axpy_f64, dX.data(), dZ_all.data(), 1.0, dX.size(), S0);  // (k == H f: the same shape)
        }
    }
    // The four implementations of one head of the backward pass.  A = X W_h and dZ are backward_layer's; the head's column block of dA_all
    // is the result.
    // delta_i = <dZ_i, out_i> of head h (= <dZ_i, o_i>: dZ is 0 where out is), the softmax's row scalar, on the compute stream; for a
    // non-ReLU layer or a layer with an addend it is what head_dz's launch for this head left in act_delta_ (a buffer of its own, which
    // nothing else writes)
    DenseMatrix& head_delta(int i, int h, const DenseMatrix& dZ) {
        if (head_act(i) != HNH_GAT_ACT_RELU || has_addend(i)) {
            if (act_delta_.rows() != dZ.rows() || act_delta_.cols() != 1)
                throw hnh::Error("Error, GAT backwardPass: the activation's delta does not have the head's rows!");
            return act_delta_;
        }
        const DenseMatrix& out = buffers[(size_t)i + 1];  // (a plain ReLU layer: never a normalised one)
        const int64_t f = dZ.cols();
        DenseMatrix& delta = scratch(SC_DELTA, dZ.rows(), 1);
        HNH_GAT_CALL(hnh_rowdot_cols_f64, delta.data(), dZ.data(), f, out.data(), out.cols(), (int64_t)h * f, dZ.rows(), f, HNH_STREAM_COMPUTE);
        return delta;
    }
    // HNH_GAT_BACKWARD_UNFUSED: seven operator calls through value vectors on the nonzeros of both layouts (allocated on first use)
    void backward_head_unfused(int i, int h, DenseMatrix& A, DenseMatrix& dZ, DenseMatrix& dA_all) {
        const int S0 = HNH_STREAM_COMPUTE;
        const bool softmax = attention_ == HNH_GAT_ATTENTION_SOFTMAX;
        const int64_t rows = A.rows(), f = A.cols();
        if (ones_S_.size() == 0) {
            ones_S_ = d_ops->like_S_values(1.0);
            ones_ST_ = d_ops->like_ST_values(1.0);
            e_S_ = VectorXd(ones_S_.size());
            d_S_ = VectorXd(ones_S_.size());
            e_ST_ = VectorXd(ones_ST_.size());
            d_ST_ = VectorXd(ones_ST_.size());
        }
        if (softmax && lse_S_.size() != ones_S_.size()) {
            lse_S_ = VectorXd(ones_S_.size());
            delta_S_ = VectorXd(ones_S_.size());
            lse_ST_ = VectorXd(ones_ST_.size());
            delta_ST_ = VectorXd(ones_ST_.size());
        }
        DenseMatrix& dArow = scratch(SC_DA_ROW, rows, f);
        DenseMatrix& T1 = scratch(SC_T1, rows, f);
        DenseMatrix& T2 = scratch(SC_T2, rows, f);
        if (softmax) {
            // lse_i and delta_i onto the nonzeros of both layouts: width-1 SDDMMs whose first operand is the S-row side in both, so S^T gets
            // the per-row scalars from the rank that owns them
            DenseMatrix& delta = head_delta(i, h, dZ);
            DenseMatrix& lse = lse_.at((size_t)i).at((size_t)h);
            if (ones_col_.rows() != rows) ones_col_ = DenseMatrix::Constant(rows, 1, 1.0);
            d_ops->setRValue(1);
            d_ops->sddmmA(lse, ones_col_, ones_S_, lse_S_);
            d_ops->sddmmA(delta, ones_col_, ones_S_, delta_S_);
            d_ops->sddmmB(lse, ones_col_, ones_ST_, lse_ST_);
            d_ops->sddmmB(delta, ones_col_, ones_ST_, delta_ST_);
            d_ops->setRValue((int)f);
        }
        // the gate: e -> a (LeakyReLU(e), or its softmax weight), da -> de
        auto gate = [&](VectorXd& e, VectorXd& d, VectorXd& lse_nz, VectorXd& delta_nz) {
            if (softmax) HNH_GAT_CALL(hnh_softmax_gate_f64, e.data(), d.data(), lse_nz.data(), delta_nz.data(), leaky_relu_alpha, e.size(), S0);
            else HNH_GAT_CALL(hnh_leaky_relu_grad_f64, e.data(), d.data(), leaky_relu_alpha, e.size(), S0);
        };
        // S layout: e_ij = <A_i, A_j>, da_ij = <dZ_i, A_j>, gate, row side dA_i = sum_j de_ij A_j
        d_ops->sddmmA(A, A, ones_S_, e_S_);
        d_ops->sddmmA(dZ, A, ones_S_, d_S_);
        gate(e_S_, d_S_, lse_S_, delta_S_);
        d_ops->spmmA(dArow, A, d_S_);
        // ST layout: the same values on the transpose's nonzeros, column sides sum_i a_ij dZ_i and sum_i de_ij A_i
        d_ops->sddmmB(A, A, ones_ST_, e_ST_);
        d_ops->sddmmB(dZ, A, ones_ST_, d_ST_);
        gate(e_ST_, d_ST_, lse_ST_, delta_ST_);
        d_ops->spmmB(dZ, T1, e_ST_);
        d_ops->spmmB(A, T2, d_ST_);
        HNH_GAT_CALL(hnh_sum3_cols_f64, dA_all.data(), dA_all.cols(), (int64_t)h * f, dArow.data(), T1.data(), T2.data(), rows, f, S0);
    }
    // HNH_GAT_BACKWARD_FUSED: two passes straight into the head's column block of dA_all (include/hnh_attn_grad.h)
    void backward_head_fused(int i, int h, DenseMatrix& A, DenseMatrix& dZ, DenseMatrix& dA_all) {
        const bool softmax = attention_ == HNH_GAT_ATTENTION_SOFTMAX;
        const int f = (int)A.cols();
        const int64_t rows = A.rows();
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);
        const double* lse = nullptr;
        const double* delta = nullptr;
        if (softmax) {
            delta = head_delta(i, h, dZ).data();
            lse = lse_.at((size_t)i).at((size_t)h).data();
        }
        const int pw = HNH_ATTN_GRAD_PACKED_WIDTH(f, softmax);
        DenseMatrix& P = scratch(SC_PACKED, rows, pw);
        HNH_GAT_CALL(hnh_attn_grad_pack_f64, P.data(), pw, A.data(), f, dZ.data(), f, lse, delta, rows, f, HNH_STREAM_COMPUTE);
        hnh_attn_grad g = {};
        g.X = A.data();
        g.ld_x = f;
        g.dZ = dZ.data();
        g.ld_dz = f;
        g.lse = lse;
        g.delta = delta;
        g.Out = dA_all.data() + (int64_t)h * f;
        g.ld_out = dA_all.cols();
        g.f = f;
        g.softmax = softmax ? 1 : 0;
        g.leaky_alpha = leaky_relu_alpha;
        bool ok = ds != nullptr && ds->attn_pass({1, g}, A, rows, true);  // row side: dA_i = sum_j de_ij A_j
        if (ok) {
            // column side onto the same rows; the moving operand is the packed one
            ScheduleWidth width(d_ops, pw, f);
            ok = ds->attn_pass({2, g}, P, rows, false);
        }
        require_own_rows("fused backward", !ok);
    }
    // score ADDITIVE (include/hnh_attn_additive.h): also the head's rows of attn_grads[i] (this rank's part)
    void backward_head_additive(int i, int h, DenseMatrix& A, DenseMatrix& dZ, DenseMatrix& dA_all) {
        const int S0 = HNH_STREAM_COMPUTE;
        const int f = layers[(size_t)i].features_per_head;
        const int64_t rows = A.rows(), hf = (int64_t)layers[(size_t)i].num_heads * f;
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);
        ensure_attn_vectors(i);
        const bool drop = attn_p_ > 0.0;  // M', Q' and the DROP instances (include/hnh_attn_dropout.h)
        const hnh_attn_drop dr = attn_drop_args(i, h);
        const int mw = drop ? HNH_ATTN_DROP_SCORED_WIDTH(f) : HNH_ATTN_ADD_SCORED_WIDTH(f), qw = HNH_ATTN_ADD_PACKED_WIDTH(f);
        DenseMatrix& M = scratch(SC_ADD_M, rows, mw);
        DenseMatrix& Q = scratch(SC_ADD_Q, rows, qw);
        DenseMatrix& D = scratch(SC_ADD_D, rows, 2);  // [ds dt]
        DenseMatrix& dAgg = scratch(SC_ADD_DAGG, rows, f);
        double* lse = lse_.at((size_t)i).at((size_t)h).data();
        head_scores(i, h, A, M, S0);
        DenseMatrix& dl = head_delta(i, h, dZ);
        if (drop) HNH_GAT_CALL(hnh_attn_drop_pack_f64, Q.data(), qw, dZ.data(), f, M.data(), mw, lse, dl.data(), rows, f, dr.row_id0, S0);
        else HNH_GAT_CALL(hnh_attn_add_pack_f64, Q.data(), qw, dZ.data(), f, M.data(), mw, lse, dl.data(), rows, f, S0);
        hnh_attn_add g = {};
        g.M = M.data();
        g.ld_m = mw;
        g.dZ = dZ.data();
        g.ld_dz = f;
        g.lse = lse;
        g.delta = dl.data();
        g.Out = dAgg.data();
        g.ld_out = f;
        g.ld_vec = 2;
        g.f = f;
        g.leaky_alpha = leaky_relu_alpha;
        bool ok = false;
        if (ds != nullptr) {  // the moving operand is M, then Q
            ScheduleWidth width(d_ops, mw, f);
            g.vec = D.data();
            ok = ds->attn_pass({1, g, drop ? &dr : nullptr}, M, rows, true);  // row side: ds
            if (ok) {
                d_ops->setRValue(qw);
                g.vec = D.data() + 1;
                ok = ds->attn_pass({2, g, drop ? &dr : nullptr}, Q, rows, true);  // column side: dAgg, dt
            }
        }
        require_own_rows("score additive", !ok);
        HNH_GAT_CALL(hnh_attn_add_update_f64, dA_all.data(), hf, (int64_t)h * f, dAgg.data(), f, D.data(), 2, attn_vector(i, h, 0), attn_vector(i, h, 1), rows, f, S0);
        // [da1_h da2_h] = A^T [ds dt] over the local rows (A = the first f columns of M)
        gemm_tn(f, 2, rows, M.data(), mw, D.data(), 2, attn_grads[(size_t)i].data() + (int64_t)h * f * 2, 2, SC_ADD_TN_WORK);
    }

    // score GATV2 (include/hnh_attn_v2.h): the pack of the fused backward, the row pass, the column pass and the dense finish, which also
    // writes the head's rows of attn_grads[i] column 0 (this rank's part)
    void backward_head_gatv2(int i, int h, DenseMatrix& A, DenseMatrix& dZ, DenseMatrix& dA_all) {
        const int S0 = HNH_STREAM_COMPUTE;
        const int f = layers[(size_t)i].features_per_head;
        const int64_t rows = A.rows(), hf = (int64_t)layers[(size_t)i].num_heads * f;
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);
        ensure_attn_vectors(i);
        const int pw = HNH_ATTN_GRAD_PACKED_WIDTH(f, 1), fe = f + (f & 1);
        DenseMatrix& P = scratch(SC_PACKED, rows, pw);
        DenseMatrix& Rm = scratch(SC_V2_R, rows, fe);
        DenseMatrix& Cm = scratch(SC_V2_C, rows, fe);
        DenseMatrix& dAgg = scratch(SC_V2_DAGG, rows, fe);
        DenseMatrix& work = scratch(SC_V2_WORK, HNH_ATTN_V2_FINISH_WORK(f), 1);
        double* lse = lse_.at((size_t)i).at((size_t)h).data();
        DenseMatrix& dl = head_delta(i, h, dZ);
        HNH_GAT_CALL(hnh_attn_grad_pack_f64, P.data(), pw, A.data(), f, dZ.data(), f, lse, dl.data(), rows, f, S0);
        hnh_attn_v2 g = {};
        g.X = A.data();
        g.ld_x = f;
        g.a = attn_vector(i, h, 0);
        g.dZ = dZ.data();
        g.ld_dz = f;
        g.lse = lse;
        g.delta = dl.data();
        g.Out = Rm.data();
        g.ld_out = fe;
        g.f = f;
        g.leaky_alpha = leaky_relu_alpha;
        bool ok = ds != nullptr && ds->attn_pass({1, g}, A, rows, true);  // row side: R
        if (ok) {
            // column side: C and dAgg; the moving operand is the packed one
            ScheduleWidth width(d_ops, pw, f);
            g.Out = Cm.data();
            g.Out2 = dAgg.data();
            g.ld_out2 = fe;
            ok = ds->attn_pass({2, g}, P, rows, true);
        }
        require_own_rows("score gatv2", !ok);
        HNH_GAT_CALL(hnh_attn_v2_finish_f64, dA_all.data(), hf, (int64_t)h * f, dAgg.data(), fe, Rm.data(), fe, Cm.data(), fe, A.data(), f, g.a,
                     attn_grads[(size_t)i].data() + (int64_t)h * f * 2, 2, rows, f, work.data(), HNH_ATTN_V2_FINISH_WORK(f), S0);
    }

    // The transformer score's operands of (layer i, head h) on the compute stream: Q = X W_q and K = X W_k into their scratch
    struct QK {
        DenseMatrix &Q, &K;
    };
    QK head_qk(int i, int h) {
        DenseMatrix& X = layer_input(i);
        const int f = layers[(size_t)i].features_per_head;
        ensure_qk_weights(i);
        QK r = {scratch(SC_QKV_Q, X.rows(), f), scratch(SC_QKV_K, X.rows(), f)};
        HNH_GAT_CALL(hnh_gemm_f64, X.rows(), f, X.cols(), X.data(), w_qk_[0][(size_t)i][(size_t)h].data(), r.Q.data(), HNH_STREAM_COMPUTE);
        HNH_GAT_CALL(hnh_gemm_f64, X.rows(), f, X.cols(), X.data(), w_qk_[1][(size_t)i][(size_t)h].data(), r.K.data(), HNH_STREAM_COMPUTE);
        return r;
    }
    // [K (0) | V (0)], the gathered operand of the forward and the row pass: the pack of the fused backward without scalars
    DenseMatrix& pack_kv(const DenseMatrix& K, const DenseMatrix& V) {
        const int f = (int)K.cols(), pw = HNH_ATTN_GRAD_PACKED_WIDTH(f, 0);
        DenseMatrix& KV = scratch(SC_QKV_KV, K.rows(), pw);
        HNH_GAT_CALL(hnh_attn_grad_pack_f64, KV.data(), pw, K.data(), f, V.data(), f, nullptr, nullptr, K.rows(), f, HNH_STREAM_COMPUTE);
        return KV;
    }
    // score TRANSFORMER (include/hnh_attn_qkv.h): Q, K and both packs, the row pass (dQ into its column block of dQ_all) and the column
    // pass (dK into dK_all, dV into dA_all: V = X W_h, so the layer's dW and dX take it as every other score's dA)
    void backward_head_transformer(int i, int h, DenseMatrix& V, DenseMatrix& dZ, DenseMatrix& dA_all, DenseMatrix& dQ_all, DenseMatrix& dK_all) {
        const int S0 = HNH_STREAM_COMPUTE;
        const int f = layers[(size_t)i].features_per_head;
        const int64_t rows = V.rows(), hf = dA_all.cols(), at = (int64_t)h * f;
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);
        const QK qk = head_qk(i, h);
        DenseMatrix& KV = pack_kv(qk.K, V);
        const int pw = HNH_ATTN_GRAD_PACKED_WIDTH(f, 1);
        DenseMatrix& P = scratch(SC_QKV_P, rows, pw);
        double* lse = lse_.at((size_t)i).at((size_t)h).data();
        DenseMatrix& dl = head_delta(i, h, dZ);
        HNH_GAT_CALL(hnh_attn_grad_pack_f64, P.data(), pw, qk.Q.data(), f, dZ.data(), f, lse, dl.data(), rows, f, S0);
        hnh_attn_qkv g = {};
        g.X = qk.Q.data();
        g.ld_x = f;
        g.dZ = dZ.data();
        g.ld_dz = f;
        g.lse = lse;
        g.delta = dl.data();
        g.Out = dQ_all.data() + at;
        g.ld_out = hf;
        g.f = f;
        g.scale = 1.0 / std::sqrt((double)f);
        bool ok = false;
        if (ds != nullptr) {  // the moving operand is [K | V], then P
            ScheduleWidth width(d_ops, (int)KV.cols(), f);
            const bool biased = edge_bias_on_[(size_t)i] != 0, learned = biased && edge_bias_learned_[(size_t)i] != 0;
            VectorXd* db[2] = {nullptr, nullptr};  // a learned bias: dL/db in S's and S^T's order, head h added to the heads before it
            if (learned)
                for (int k = 0; k < 2; k++) {
                    VectorXd& d = dbias_[k][(size_t)i];
                    if (d.size() != edge_bias_[k][(size_t)i].size()) d = VectorXd(edge_bias_[k][(size_t)i].size());
                    db[k] = &d;
                }
            auto with_edge = [&](hnh::AttnPass pass, int k) {  // (S's order for the row pass, S^T's for the column pass)
                pass.bias = biased ? &edge_bias_[k][(size_t)i] : nullptr;
                pass.dbias = db[k];
                pass.accumulate = h > 0;
                return pass;
            };
            ok = ds->attn_pass(with_edge({1, g}, 0), KV, rows, true);  // row side: dQ
            if (ok) {
                d_ops->setRValue(pw);
                g.X = qk.K.data();
                g.X2 = V.data();
                g.ld_x2 = f;
                g.Out = dK_all.data() + at;
                g.Out2 = dA_all.data() + at;
                g.ld_out2 = hf;
                ok = ds->attn_pass(with_edge({2, g}, 1), P, rows, true);  // column side: dK, dV
                if (ok && learned && h + 1 == layers[(size_t)i].num_heads) dbias_held_[(size_t)i] = 1;
            }
        }
        require_own_rows("score transformer", !ok);
    }

    DenseMatrix product[2];  // X * W_j of the head in flight and of the next one
    void* ev_input = nullptr;
    void* ev_gemm[2] = {nullptr, nullptr};
    void* ev_head[2] = {nullptr, nullptr};

    void shape_product(int i, DenseMatrix& A) { shaped(A, buffers[i].rows(), layers[i].wMats[0].cols()); }

    // the softmax passes' row state: the running max / sum of `rows` rows (shared by the heads) and the lse vector of (layer i, head j)
    DenseMatrix& softmax_row_state(int i, int j, int64_t rows) {
        if (row_max_.rows() != rows) {
            row_max_ = DenseMatrix(rows, 1);
            row_sum_ = DenseMatrix(rows, 1);
        }
        if (lse_.size() != layers.size()) lse_.assign(layers.size(), std::vector<DenseMatrix>());
        std::vector<DenseMatrix>& lse = lse_[(size_t)i];
        if (lse.size() != (size_t)layers[i].num_heads) lse.assign((size_t)layers[i].num_heads, DenseMatrix());
        if (lse[(size_t)j].rows() != rows) lse[(size_t)j] = DenseMatrix(rows, 1);
        return lse[(size_t)j];
    }

    void shape_scored(int i, DenseMatrix& M) {
        const int f = layers[i].features_per_head;
        shaped(M, buffers[i].rows(), attn_p_ > 0.0 ? HNH_ATTN_DROP_SCORED_WIDTH(f) : HNH_ATTN_ADD_SCORED_WIDTH(f));
    }

    // The scored operand of (layer i, head j) from the head's product A, on `stream`: M = [A (0) | <A, a1_j> <A, a2_j>]
    // (include/hnh_attn_additive.h) or, with attention dropout, M' = [A (0) | s t | id 0] at M's own width
    void head_scores(int i, int j, DenseMatrix& A, DenseMatrix& M, int stream) {
        const int f = layers[i].features_per_head;
        const double *a1 = attn_vector(i, j, 0), *a2 = attn_vector(i, j, 1);
        if (attn_p_ > 0.0)
            HNH_GAT_CALL(hnh_attn_drop_scores_f64, M.data(), M.cols(), A.data(), A.cols(), a1, a2, A.rows(), f, d_ops->aSubmatrices[0].topRow, stream);
        else HNH_GAT_CALL(hnh_attn_add_scores_f64, M.data(), M.cols(), A.data(), A.cols(), a1, a2, A.rows(), f, stream);
    }

    // A = buffers[i] * W_j (gat.hpp:88) on `stream`
    void head_product(int i, int j, DenseMatrix& A, int stream) {
        DenseMatrix& X = layer_input(i);
        DenseMatrix& W = layers[i].wMats[j];
        if (X.cols() != W.rows()) hnh::fatal("Error, GAT weight shape does not match the layer input!");
        shape_product(i, A);
        HNH_GAT_CALL(hnh_gemm_f64, X.rows(), W.cols(), X.cols(), X.data(), W.data(), A.data(), stream);
    }

    // What the three scores' softmax passes share for one head: the row state and the head's lse vector (softmax_row_state), the carrier H
    // of the unnormalised rows between the launches of the pass (allocated here, per head, on the compute stream), the head's column block
    // of the layer output, and the finishing launch's activation and addend flags.
    struct SoftmaxHead {
        DenseMatrix H;
        double *lse, *row_max, *row_sum, *dst;
        int64_t ld_dst;
        int f;
        double leaky_alpha;
        unsigned flags;
        template <class Args>
        void fill(Args& g) const {  // the members hnh_attn_add and hnh_attn_v2 have in common
            g.lse = lse;
            g.Out = H.data();
            g.ld_out = H.cols();
            g.row_max = row_max;
            g.row_sum = row_sum;
            g.relu_dst = dst;
            g.relu_ld = ld_dst;
            g.f = f;
            g.leaky_alpha = leaky_alpha;
        }
    };
    SoftmaxHead softmax_head(int i, int j, int64_t rows, int64_t carrier_cols) {
        DenseMatrix& out = head_target(i);
        const int f = layers[i].features_per_head;
        double* lse = softmax_row_state(i, j, rows).data();
        return {DenseMatrix(rows, carrier_cols), lse, row_max_.data(), row_sum_.data(), out.data() + (int64_t)j * f, out.cols(), f, leaky_relu_alpha,
                activation_flag(i) | addend_flag(i)};
    }

    // the rest of the head (gat.hpp:89-101) from its product A, on the compute stream; A is consumed (the unfused route zeroes it)
    void head_attention(int i, int j, DenseMatrix& A) {
        const int f = layers[i].features_per_head;
        d_ops->setRValue(f);
        DenseMatrix& out = buffers[i + 1];
        auto* ds = dynamic_cast<Sparse15D_Dense_Shift*>(d_ops);

        if (score_ == HNH_GAT_SCORE_ADDITIVE) {
            // A is the scored operand M = [A (0) | s t]: one pass that gathers one row of M per nonzero (include/hnh_attn_additive.h), with
            // the softmax pass's row state; the schedule runs at M's width for it
            const SoftmaxHead s = softmax_head(i, j, A.rows(), f + (f & 1));
            hnh_attn_add g = {};
            g.M = A.data();
            g.ld_m = A.cols();
            s.fill(g);
            bool ok = false;
            if (ds != nullptr) {
                ScheduleWidth width(d_ops, (int)A.cols(), f);
                const hnh_attn_drop dr = attn_drop_args(i, j);
                ok = ds->attn_pass({0, g, attn_p_ > 0.0 ? &dr : nullptr, s.flags}, A, A.rows(), true);
            }
            require_own_rows("score additive", !ok);
            return;
        }
        if (score_ == HNH_GAT_SCORE_GATV2) {
            // one pass on the plain product with the softmax pass's row state (include/hnh_attn_v2.h): the schedule runs at the head's f
            const SoftmaxHead s = softmax_head(i, j, A.rows(), f + (f & 1));
            hnh_attn_v2 g = {};
            g.X = A.data();
            g.ld_x = A.cols();
            g.a = attn_vector(i, j, 0);
            s.fill(g);
            require_own_rows("score gatv2", ds == nullptr || !ds->attn_pass({0, g, nullptr, s.flags}, A, A.rows(), true));
            return;
        }
        if (score_ == HNH_GAT_SCORE_TRANSFORMER) {
            // A is V; Q and K are made here, on the compute stream, and one pass gathers the packed [K | V] with the softmax pass's row
            // state (include/hnh_attn_qkv.h): the schedule runs at the packed width
            const SoftmaxHead s = softmax_head(i, j, A.rows(), f + (f & 1));
            const QK qk = head_qk(i, j);
            DenseMatrix& KV = pack_kv(qk.K, A);
            hnh_attn_qkv g = {};
            g.X = qk.Q.data();
            g.ld_x = f;
            g.lse = s.lse;
            g.Out = const_cast<double*>(s.H.data());
            g.ld_out = s.H.cols();
            g.row_max = s.row_max;
            g.row_sum = s.row_sum;
            g.relu_dst = s.dst;
            g.relu_ld = s.ld_dst;
            g.f = f;
            g.scale = 1.0 / std::sqrt((double)f);
            bool ok = false;
            if (ds != nullptr) {
                ScheduleWidth width(d_ops, (int)KV.cols(), f);
                hnh::AttnPass pass = {0, g, nullptr, s.flags};
                pass.bias = edge_bias_on_[(size_t)i] ? &edge_bias_[0][(size_t)i] : nullptr;
                ok = ds->attn_pass(pass, KV, A.rows(), true);
            }
            require_own_rows("score transformer", !ok);
            return;
        }
        if (attention_ == HNH_GAT_ATTENTION_SOFTMAX) {
            // one fused pass with the online softmax (include/hnh_attention.h): the head's activated output leaves the finishing launch
            // straight into its column block, lse into this head's vector; H carries the unnormalised rows between the launches
            SoftmaxHead s = softmax_head(i, j, A.rows(), A.cols());
            const hnh_attn_state st = {s.row_max, s.row_sum, s.lse, leaky_relu_alpha, s.dst, s.ld_dst};
            require_own_rows("softmax attention", ds == nullptr || !ds->fusedSoftmax_out(A, A, Amat, s.H, st, s.flags));
            return;
        }

        // Schedules with a single fused pass (1.5D dense shift, local kernel fusion, c = 1: its shifts are empty and
        // the attention matrix is not exported) do SDDMM, LeakyReLU and SpMM in ONE gather of the neighbours' rows.
        if (d_ops->c == 1) {
            // ... and the head's ReLU output (gat.hpp:101) leaves the same launch straight into its column block of the layer
            // output: H only carries partial sums between the launches of a pass
            DenseMatrix H(A.rows(), A.cols());
            hnh_fused_extras ex = {leaky_relu_alpha, 0.0, nullptr, nullptr, out.data() + (int64_t)j * A.cols(), (int64_t)out.cols()};
            if (d_ops->fusedSpMM_out(A, A, Amat, H, true, ex)) return;
        }

        VectorXd Svalues = d_ops->like_S_values(1.0);
        VectorXd sddmm_buffer = d_ops->like_S_values(1.0);
        DenseMatrix B = A;
        d_ops->de_shift(&B, nullptr, k_spmmA);

        d_ops->algorithm(A, B, Svalues, &sddmm_buffer, k_sddmmA, true);  // SDDMM phase
        A.setZero();
        HNH_GAT_CALL(hnh_leaky_relu_f64, sddmm_buffer.data(), leaky_relu_alpha, sddmm_buffer.size(), HNH_STREAM_COMPUTE);
        d_ops->algorithm(A, B, sddmm_buffer, nullptr, k_spmmA, false);   // SpMM phase, replication reused
        HNH_GAT_CALL(hnh_relu_store_cols_f64, out.data(), out.cols(), (int64_t)j * A.cols(), A.data(), A.rows(), A.cols(), HNH_STREAM_COMPUTE);
    }
};
#undef HNH_GAT_KERNEL
#undef HNH_GAT_CALL
