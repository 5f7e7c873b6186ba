"""The export of the GAT's attention coefficients without a GPU: the single-pass reference (tests/gat_coef_ref.py) against the model's trace
in every mode, its row sums, its conditioning on the kernel tests' operands (float64 against np.longdouble), the optional kernel group of
include/hnh_attn_coef.h (declared == bound == exported by the HIP library, disjoint from the seven existing tables, absent from the CPU test
double), the host call, every refusal on the test double (nothing in flight, the plain GAT on the same object bit-equal to an untouched one),
and DistributedSparse.S_coordinates / ST_coordinates on five schedules, where they use existing kernels only."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_coef_ref as CR
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, plain_output
from gat_gpu_harness import FTOL, graph, mixed_degrees
from oracle import oracle as O

GROUP = {"hnh_attn_coef_csr_p", "hnh_attn_coef_scores_f64"}
WIDTHS = [1, 7, 8, 33, 64, 100, 128, 200, 255, 256]
MODES = [("dot", (0.0, 0.0)), ("additive", (0.0, 0.0)), ("additive", (0.6, 0.3)), ("gatv2", (0.0, 0.0))]


@pytest.mark.parametrize("activations", ["relu", ("elu", "identity")])
@pytest.mark.parametrize("score,rates", MODES)
def test_pass_reference_equals_the_models_trace(score, rates, activations):
    rows, cols, m, x, w, av, _ = fd_problem()
    mode = dict(activations=activations, rates=rates, seed=11) if rates != (0.0, 0.0) else dict(activations=activations)
    tr = CR.model_trace(score, rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, w, av, **mode)
    ids = np.arange(m)
    for (li, h), t in tr.items():
        a_mat = t["A"]
        if score == "additive":
            xo, yo, vec = a_mat @ av[(li, h)][0], a_mat @ av[(li, h)][1], None
        else:
            xo, yo, vec = a_mat, a_mat, (av[(li, h)][0] if score == "gatv2" else None)
        got = CR.coef_pass(rows, cols, xo, yo, t["lse"], score, T.GAT_ALPHA, vec)
        assert T.rel(got, t["a"]) <= 1e-13, (li, h, T.rel(got, t["a"]))
        if rates[0] > 0.0:
            drop = (11, li * 65536 + h, rates[0], ids, ids)
            got = CR.coef_pass(rows, cols, xo, yo, t["lse"], score, T.GAT_ALPHA, vec, drop=drop)
            assert np.any(t["ck"] == 0) and np.any(t["ck"] > 0)
            assert T.rel(got, t["a"] * t["ck"]) <= 1e-13 and np.array_equal(got == 0, t["ck"] == 0)
        ld = CR.coef_pass_ld(rows, cols, xo, yo, t["lse"], score, T.GAT_ALPHA, vec)
        assert ld.dtype == np.longdouble and T.rel(np.float64(ld), t["a"]) <= 1e-13


def kernel_block(f, seed=0, m=2048, ncols=1536):
    """The block of the GPU kernel tests: mixed_degrees (empty rows, rows of 200 - 300, hub rows of 600 and 1500) and a planted repeated pair"""
    rowptr, colidx, rows = graph(m, ncols, mixed_degrees(m, seed + f), seed + 1)
    return rowptr, colidx, rows, colidx.astype(np.int64), m, ncols


@pytest.mark.parametrize("score", CR.SCORES)
def test_rows_of_the_reference_sum_to_one(score):
    rowptr, colidx, rows, cols, m, ncols = kernel_block(33)
    assert np.diff(rowptr).max() == 1500 and np.any(np.diff(rowptr) == 0)
    o = CR.with_lse(CR.operands(score, 33, rows, cols, m, ncols), rows, cols, m, score, T.GAT_ALPHA)
    sums = CR.row_sums(rows, m, CR.coef_pass(rows, cols, o["x"], o["y"], o["lse"], score, T.GAT_ALPHA, o["a"]))
    live = np.diff(rowptr) > 0
    assert np.max(np.abs(sums[live] - 1.0)) <= T.TOL and np.all(sums[~live] == 0.0)
    assert abs(sums[m // 2] - 1.0) <= T.TOL  # the 1500-nonzero row


@pytest.mark.parametrize("score", CR.SCORES)
def test_float64_reference_is_well_inside_the_kernel_bound_on_the_kernel_tests_operands(score):
    """Conditioning: on the operands the GPU tests use, the float64 pass stays within FTOL / 10 of the longdouble one at every tested width, so
    the bound the kernel is held to (FTOL) is met by the reference alone with a factor of ten to spare."""
    worst = 0.0
    for f in WIDTHS:
        rowptr, colidx, rows, cols, m, ncols = kernel_block(f)
        o = CR.with_lse(CR.operands(score, f, rows, cols, m, ncols), rows, cols, m, score, T.GAT_ALPHA)
        v64 = CR.coef_pass(rows, cols, o["x"], o["y"], o["lse"], score, T.GAT_ALPHA, o["a"])
        vld = CR.coef_pass_ld(rows, cols, o["x"], o["y"], o["lse"], score, T.GAT_ALPHA, o["a"])
        err = float(T.rel(np.asarray(v64, dtype=np.longdouble), vld))
        worst = max(worst, err)
        assert err <= FTOL / 10, (score, f, err)
    T.record_observed("gat_coef_reference_conditioning", score=score, worst=worst)


def test_coef_kernels_are_an_optional_group():
    names = declared("hnh_attn_coef.h")
    assert names == GROUP
    assert names == set(K.ATTN_COEF_SIGNATURES), names ^ set(K.ATTN_COEF_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_attn_additive.h", "hnh_attn_dropout.h", "hnh_train.h",
                   "hnh_attn_v2.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES, K.ATTN_ADD_SIGNATURES, K.ATTN_DROP_SIGNATURES,
                  K.TRAIN_SIGNATURES, K.V2_SIGNATURES):
        assert not names & set(table), "disjoint from the existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.ATTN_COEF_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.AttnCoef) == 72  # struct hnh_attn_coef: seven pointers and pitches, two ints, a double
    txt = open(ROOT + "/include/hnh_attn_coef.h").read()
    assert re.search(r"#define HNH_ATTN_COEF_MAX_F %d\b" % K.ATTN_COEF_MAX_F, txt)
    assert re.search(r"#define HNH_ATTN_COEF_PAIR_WIDTH %d\b" % K.ATTN_COEF_PAIR_WIDTH, txt)
    for name, code in CR.SCORE_CODE.items():
        assert re.search(r"#define HNH_ATTN_COEF_%s %d\b" % (name.upper(), code), txt)
    assert (K.ATTN_COEF_DOT, K.ATTN_COEF_ADDITIVE, K.ATTN_COEF_GATV2) == (0, 1, 2)


def test_host_wiring():
    txt = open(ROOT + "/include/hnh_dist.h").read()
    assert re.search(r"int hnh_gat_attention_coefficients\(hnh_gat\* g, int layer, int head, int dropped, hnh_vec\* out\);", txt)
    assert "hnh_gat_attention_coefficients" in H.SIGNATURES
    assert H.lib().hnh_gat_attention_coefficients is not None
    assert callable(H.GAT.attention_coefficients) and callable(H.DistributedSparse.S_coordinates) and callable(H.DistributedSparse.ST_coordinates)


# ------------------------------------------------------------------------------------------------ refusals on the test double
def refused(case, words, ranks=1, alg="15d_fusion2", c=1, layers=None, prepare=None, call=None, **kw):
    """attention_coefficients raises HnhError matching `words` (prepare(gnn, world) runs first; call(gnn, d) makes the call); nothing is in
    flight afterwards (a device synchronisation through a download succeeds), and the plain GAT on the same object is bit-equal to that of
    an object that never heard of the export (schedules on which the plain GAT is the reference's only)."""
    def rank(world):
        sp, d, gnn = make_gat(world, case, alg, c, layers=layers, **dict(dict(attention="softmax"), **kw))
        r0 = d.info()["R"]
        if prepare is not None:
            prepare(gnn, world)
        with pytest.raises(H.HnhError, match=words) as e:
            if call is not None:
                call(gnn, d)
            else:
                gnn.attention_coefficients(0, 0)
        msg = str(e.value)
        assert d.info()["R"] == r0, "a refusal leaves the operator's R alone"
        res = None
        if layers is None and alg == "15d_fusion2" and c == 1:
            gnn.set_score("dot")
            gnn.set_attention("none")
            gnn.set_dropout(0.0, 0.0, 0)
            gnn.forwardPass()
            out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
            gnn.get_output(out)
            res = out.download()
            out.free()
        for h in (gnn, d, sp):
            h.free()
        return msg, res

    per_rank = H.run_spmd(ranks, rank)
    if per_rank[0][1] is not None:
        want = H.run_spmd(ranks, lambda world: plain_output(world, case))
        assert all(np.isfinite(r[1]).all() and np.array_equal(r[1], b) for r, b in zip(per_rank, want))
    return per_rank[0][0]


def test_refused_before_any_forward_pass_and_after_set_weight():
    """On the test double the kernel group is absent, and the checks come in the project's order (arguments, mode, schedule, width, kernel group,
    then the stored pass, as in backwardPass): the refusal names the group.  With attention none, where a forward pass runs on the test double,
    the mode is refused by name whether a forward pass is stored, has been invalidated by set_weight, or never ran."""
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    refused(case, r"attention_coefficients.*hnh_attn_coef_csr_p.*include/hnh_attn_coef\.h")
    refused(case, "attention_coefficients.*attention mode softmax only.*attention mode none", attention="none")
    refused(case, "attention_coefficients.*attention mode none", attention="none", prepare=lambda g, w: g.forwardPass())

    def invalidate(g, w):
        g.forwardPass()
        g.set_weight(0, 0, np.zeros(g.weight_shape(0, 0)))
    refused(case, "attention_coefficients.*attention mode none", attention="none", prepare=invalidate)


def test_refuses_bad_arguments():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    refused(case, "layer index 2 out of range", call=lambda g, d: g.attention_coefficients(2, 0))
    refused(case, "layer index -1 out of range", call=lambda g, d: g.attention_coefficients(-1, 0))
    refused(case, "head index 3 out of range", call=lambda g, d: g.attention_coefficients(1, 3))
    refused(case, "head index 2 out of range", call=lambda g, d: g.attention_coefficients(0, 2))

    def short(g, d):
        like = d.like_S_values(0.0)
        v = H.Vec.create(d.w, len(like) + 1)
        like.free()
        try:
            g.attention_coefficients(0, 0, out=v)
        finally:
            v.free()
    refused(case, "like_S_values length", call=short)


@pytest.mark.parametrize("alg,p,c,name", [("15d_fusion1", 4, 2, "15d_fusion1"), ("15d_fusion2", 4, 2, "15d_fusion2")])
def test_refuses_unsupported_schedules(alg, p, c, name):
    H.load_backend(T.ORACLE_BACKEND)
    refused(T.case_inputs("er8_r16"), "attention_coefficients.*%s.*c = %d" % (name, c), ranks=p, alg=alg, c=c, layers=[(16, 8, 2)])


def test_refuses_wide_heads_and_a_head_of_256_reaches_the_kernel_check():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    refused(case, "attention_coefficients.*at most 256 features, not 257", layers=[(16, 257, 1)])
    refused(case, r"hnh_attn_coef_csr_p.*include/hnh_attn_coef\.h", layers=[(16, 256, 1)])


# ------------------------------------------------------------------------------------------------ coordinates
CONFIGS = [(alg, p, c) for alg in ("15d_fusion1", "15d_fusion2", "15d_sparse", "25d_dense_replicate", "25d_sparse_replicate")
           for (p, c) in ((1, 1), (2, 1), (4, 1), (4, 2), (8, 2)) if T.valid_config(alg, p, c, 16)]


@pytest.mark.parametrize("alg,p,c", CONFIGS)
def test_coordinates_cover_every_edge_once_and_index_the_sddmm(alg, p, c):
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    n = case["N"]

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], n, case["rows"], case["cols"], case["vals"])
        d = H.DistributedSparse(world, alg, sp, case["R"], c)
        r0 = d.info()["R"]
        sr, sc = d.S_coordinates()
        tr, tc = d.ST_coordinates()
        assert d.info()["R"] == r0, "the operator's R is unchanged"
        assert sr.dtype == np.int64 and sc.dtype == np.int64 and len(sr) == len(d.like_S_values(0.0)) and len(tr) == len(d.like_ST_values(0.0))
        # sddmmA with S = 1 in this layout
        A, B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
        A.upload(T.fill_local(d.submatrices(H.AMAT), A.shape, case["A"]))
        B.upload(T.fill_local(d.submatrices(H.BMAT), B.shape, case["B"]))
        ones, res = d.like_S_values(1.0), d.like_S_values(0.0)
        d.initial_shift(A, B, H.K_SDDMM_A)
        d.sddmmA(A, B, ones, res)
        vals = res.download()
        for x in (A, B, ones, res, d, sp):
            x.free()
        return sr, sc, tr, tc, vals

    per_rank = H.run_spmd(p, rank)
    want = np.sort(case["rows"] * n + case["cols"])
    assert len(np.unique(want)) == len(want)
    keys = np.concatenate([r[0] * n + r[1] for r in per_rank])
    assert np.array_equal(np.sort(keys), want), "every edge exactly once"
    keys_t = np.concatenate([r[3] * n + r[2] for r in per_rank])  # (ST_coordinates: rows are columns of S)
    assert np.array_equal(np.sort(keys_t), want), "every edge of the transpose exactly once"
    tkeys = np.concatenate([r[2] * case["M"] + r[3] for r in per_rank])
    assert np.array_equal(np.sort(tkeys), np.sort(case["cols"] * case["M"] + case["rows"])), "the transposed edge set"
    rows = np.concatenate([r[0] for r in per_rank])
    cols = np.concatenate([r[1] for r in per_rank])
    got = np.concatenate([r[4] for r in per_rank])
    ref = O.sddmm_local(rows, cols, np.zeros(len(rows)), case["A"], case["B"])
    assert T.rel(got, ref) <= T.TOL, T.rel(got, ref)
