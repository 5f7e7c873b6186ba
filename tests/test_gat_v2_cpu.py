"""The GAT's score "gatv2" without a GPU: the numpy definition (tests/gat_v2_ref.py) against central finite differences, its pass-level
restatement against the definition (with the identity da = colsum(A o (R + C))), a hand-made example on which the attention is dynamic where
the additive score's cannot be, the optional kernel group of include/hnh_attn_v2.h (declared == bound == exported by the HIP library, disjoint
from the six existing tables, absent from the CPU test double), the host calls, and on the test double: score "gatv2" names a kernel of the
new group and its header, every unsupported shape is refused by name before any launch, and a plain GAT on the same object runs as before."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_ref as R
import gat_v2_ref as V
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, plain_output

GROUP = {"hnh_attn_v2_fwd_csr_p", "hnh_attn_v2_row_csr_p", "hnh_attn_v2_col_csr_p", "hnh_attn_v2_finish_f64"}
STEP = 1e-6


def fd_inputs(activations):
    """fd_problem() with x drawn again from the first seed at which every u_ijc = A_ic + A_jc of every head and every aggregate lies at
    least 100 steps from 0: the kinks sit per edge and per feature here, so the seed is chosen on the CPU and the condition asserted."""
    rows, cols, m, x, w, av, g = fd_problem()
    a = {k: v[0] for k, v in av.items()}
    for seed in range(200):
        xs = np.random.default_rng(1000 + seed).uniform(-1, 1, x.shape)
        pre = V.pre_activations(rows, cols, m, xs, T.GAT_LAYERS, T.GAT_ALPHA, w, a, activations=activations)
        if np.abs(pre).min() >= 200 * STEP:
            return rows, cols, m, xs, w, a, g
    raise AssertionError("no seed keeps every kink 200 steps away")


@pytest.mark.parametrize("activations", ["relu", ("elu", "identity")])
def test_reference_backward_matches_finite_differences(activations):
    rows, cols, m, x, w, av, g = fd_inputs(activations)
    layers, alpha = T.GAT_LAYERS, T.GAT_ALPHA
    mode = dict(activations=activations)
    dws, das, dx = V.backward(rows, cols, m, x, layers, alpha, g, w, av, **mode)

    def loss(ww, aa, xx):
        return float(np.sum(g * V.forward(rows, cols, m, xx, layers, alpha, ww, aa, **mode)))

    def margin_ok(ww, aa, xx, steps=100):
        return np.abs(V.pre_activations(rows, cols, m, xx, layers, alpha, ww, aa, **mode)).min() >= steps * STEP

    assert margin_ok(w, av, x), "every |A_ic + A_jc| and every pre-activation is at least 100 steps from 0"
    assert all(np.all(d != 0) for d in das.values()), "every entry of da is non-zero"
    assert np.count_nonzero(dx) > dx.size // 2 and all(np.abs(d).max() > 0 for d in dws.values()), "the gradients must not be vacuous"

    def fd_of(perturb, probes):
        out = []
        for idx in probes:
            plus, minus = perturb(idx, STEP), perturb(idx, -STEP)
            assert margin_ok(*plus, steps=99) and margin_ok(*minus, steps=99)
            out.append((loss(*plus) - loss(*minus)) / (2 * STEP))
        return np.array(out)

    rng = np.random.default_rng(3)
    for key, wk in w.items():  # every dW
        probes = [(0, 0), (wk.shape[0] - 1, wk.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in wk.shape) for _ in range(3)]

        def perturb(idx, h, key=key, wk=wk):
            ww = dict(w)
            ww[key] = wk.copy()
            ww[key][idx] += h
            return ww, av, x

        an = np.array([dws[key][idx] for idx in probes])
        err = np.max(np.abs(fd_of(perturb, probes) - an)) / np.max(np.abs(an))
        assert err <= 1e-6, (key, err)
    for key, a in av.items():  # every entry of every da
        def perturb(idx, h, key=key):
            aa = dict(av)
            aa[key] = av[key].copy()
            aa[key][idx] += h
            return w, aa, x

        an = das[key]
        err = np.max(np.abs(fd_of(perturb, list(range(len(a)))) - an)) / np.max(np.abs(an))
        assert err <= 1e-6, (key, err)
    probes = [(0, 0), (m - 1, x.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in x.shape) for _ in range(4)]

    def perturb_x(idx, h):
        xx = x.copy()
        xx[idx] += h
        return w, av, xx

    an = np.array([dx[idx] for idx in probes])
    err = np.max(np.abs(fd_of(perturb_x, probes) - an)) / np.max(np.abs(an))
    assert err <= 1e-6, err


@pytest.mark.parametrize("activations", ["relu", ("elu", "identity")])
def test_passes_with_the_packed_operand_equal_the_definition(activations):
    rows, cols, m, x, w, av, g = fd_inputs(activations)
    want = V.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, av, activations=activations)
    got = V.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, av, activations=activations, by_passes=True)
    for k in want[0]:
        assert T.rel(got[0][k], want[0][k]) <= T.TOL
        assert T.rel(got[1][k], want[1][k]) <= T.TOL, "da = colsum(A o (R + C)) is the direct sum_ij g_ij LReLU(u_ij)"
    assert T.rel(got[2], want[2]) <= T.TOL
    # the forward pass as the kernel takes it, and its extended-precision twin
    fin, f, _ = T.GAT_LAYERS[0]
    a_mat = x @ w[(0, 0)]
    o, lse, z, _ = V.fwd_pass(rows, cols, m, a_mat, a_mat, av[(0, 0)], f, T.GAT_ALPHA)
    _, trace = V.forward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, w, av, activations=activations, keep_trace=True)
    assert T.rel(o, trace[0][3][0][3]) <= T.TOL and T.rel(lse, trace[0][3][0][4]) <= T.TOL
    o_ld, lse_ld = V.fwd_pass_ld(rows, cols, m, a_mat, a_mat, av[(0, 0)], f, T.GAT_ALPHA)
    assert o_ld.dtype == np.longdouble and T.rel(np.float64(o_ld), o) <= 1e-13 and T.rel(np.float64(lse_ld), lse) <= 1e-13


def test_the_identity_for_da_on_its_own():
    """sum_ij g_ij LReLU(A_i + A_j) = colsum(A o R) + colsum(A o C) for ANY per-nonzero weights g, a repeated pair included"""
    rng = np.random.default_rng(0)
    m, f, alpha = 9, 5, 0.2
    rows, cols = rng.integers(0, m, 40), rng.integers(0, m, 40)
    rows[1], cols[1] = rows[0], cols[0]
    a_mat, gij = rng.standard_normal((m, f)), rng.standard_normal(40)
    u = a_mat[rows] + a_mat[cols]
    sg = np.where(u > 0, 1.0, alpha)
    rm, cm = np.zeros((m, f)), np.zeros((m, f))
    np.add.at(rm, rows, gij[:, None] * sg)
    np.add.at(cm, cols, gij[:, None] * sg)
    assert T.rel(np.sum(a_mat * (rm + cm), axis=0), gij @ R.leaky(u, alpha)) <= 1e-13


def test_gatv2_is_dynamic_where_additive_is_static():
    """Two rows that share two neighbours: under GATv2 row 0 prefers neighbour 0 and row 1 prefers neighbour 1; under the additive score
    LReLU(s_i + t_j) is monotone in t_j, so every row ranks the neighbours alike, whatever a1, a2 are."""
    alpha = 0.2
    keys = np.array([[1.0, 0.0], [0.0, 1.0]])     # A_j of neighbour 0, 1
    queries = np.array([[-1.0, 0.0], [0.0, -1.0]])  # A_i of row 0, 1
    a = np.array([-1.0, -1.0])
    z = np.array([[R.leaky(q + k, alpha) @ a for k in keys] for q in queries])
    assert z[0, 0] > z[0, 1] and z[1, 1] > z[1, 0], z
    # the same through the pass reference: rows 0, 1 of a 2 x 2 block with both nonzeros each
    rows, cols = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
    _, _, zz, p = V.fwd_pass(rows, cols, 2, queries, keys, a, 2, alpha)
    assert np.array_equal(zz.reshape(2, 2), z) and p[0] > p[1] and p[3] > p[2]
    rng = np.random.default_rng(4)
    for _ in range(200):  # additive: the ranking of the neighbours is the same for both rows
        a1, a2 = rng.standard_normal(2) * 3, rng.standard_normal(2) * 3
        e = R.leaky((queries @ a1)[:, None] + (keys @ a2)[None, :], alpha)
        assert np.sign(e[0, 0] - e[0, 1]) == np.sign(e[1, 0] - e[1, 1])


def test_forward_is_finite_far_outside_exps_range():
    from oracle import oracle as O
    rows, cols = O.erdos_renyi(6, 8)
    m, f = 64, 6
    rng = np.random.default_rng(1)
    a_mat = rng.uniform(-1, 1, (m, f))
    o, lse, z, _ = V.fwd_pass(rows, cols, m, a_mat, a_mat, rng.uniform(-1, 1, f) * 600, f, T.GAT_ALPHA)
    assert np.abs(z).max() > 800 and np.all(np.isfinite(o)) and np.all(np.isfinite(lse))


def test_v2_kernels_are_an_optional_group():
    names = declared("hnh_attn_v2.h")
    assert names == GROUP
    assert names == set(K.V2_SIGNATURES), names ^ set(K.V2_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_attn_additive.h", "hnh_attn_dropout.h", "hnh_train.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES, K.ATTN_ADD_SIGNATURES, K.ATTN_DROP_SIGNATURES,
                  K.TRAIN_SIGNATURES):
        assert not names & set(table), "disjoint from the existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.V2_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.AttnV2) == 152  # struct hnh_attn_v2: seventeen pointers and pitches, an int (padded), a double
    txt = open(ROOT + "/include/hnh_attn_v2.h").read()
    assert re.search(r"#define HNH_ATTN_V2_MAX_F %d\b" % K.ATTN_V2_MAX_F, txt)
    assert re.search(r"#define HNH_ATTN_V2_FINISH_WORK\(f\) \(1024 \* \(int64_t\)\(f\)\)", txt) and K.attn_v2_finish_work(7) == 7168


def test_host_wiring():
    txt = open(ROOT + "/include/hnh_dist.h").read()
    assert re.search(r"#define HNH_GAT_SCORE_GATV2 2\b", txt) and re.search(r"#define HNH_GAT_SCORE_ADDITIVE 1\b", txt)
    assert H.GAT.SCORE == {"dot": 0, "additive": 1}, "the existing table is unchanged"
    assert H.GAT.SCORE_V2 == {"gatv2": 2}
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, attention="softmax")
        gnn.set_score("gatv2")
        with pytest.raises(ValueError, match="additive.*dot.*gatv2"):
            gnn.set_score("bilinear")
        assert H.lib().hnh_gat_set_score(gnn.h, 2) == 0 and H.lib().hnh_gat_set_score(gnn.h, 7) != 0
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(1, rank))


def refused(case, words, ranks=1, alg="15d_fusion2", c=1, layers=None, backward=True, **kw):
    """forwardPass (and backwardPass) of a gatv2 GAT raise HnhError matching `words`; the same object then runs a plain GAT whose output is
    bit-equal to that of an object that never heard of the score (schedules on which the plain GAT is the reference's only)."""
    def rank(world):
        sp, d, gnn = make_gat(world, case, alg, c, layers=layers, **dict(dict(attention="softmax", score="gatv2"), **kw))
        with pytest.raises(H.HnhError, match=words) as e:
            gnn.forwardPass()
        msg = str(e.value)
        if backward:
            g = H.Dense.create(world, *gnn.buffer_shape(len(layers or T.GAT_LAYERS)))
            with pytest.raises(H.HnhError, match=words):
                gnn.backwardPass(g)
            g.free()
        res = None
        if layers is None and alg == "15d_fusion2" and c == 1:
            gnn.set_score("dot")  # the process and the operator live on: the plain GAT on the same object
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


def test_gatv2_on_the_test_double_names_the_missing_kernel():
    H.load_backend(T.ORACLE_BACKEND)
    msg = refused(T.case_inputs("er8_r16"), r"gatv2.*hnh_attn_v2_[a-z0-9_]+.*include/hnh_attn_v2\.h", ranks=2)
    assert re.search(r"hnh_attn_v2_[a-z0-9_]+", msg).group(0) in GROUP


def test_gatv2_refuses_attention_none_and_attention_dropout():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    refused(case, "score gatv2.*attention mode softmax only.*attention mode none", attention="none")
    refused(case, "attention dropout.*gatv2", dropout=(0.25, 0.0), seed=3)


@pytest.mark.parametrize("alg,p,c,name", [("15d_fusion1", 4, 2, "15d_fusion1"), ("15d_fusion2", 4, 2, "15d_fusion2")])
def test_gatv2_refuses_unsupported_schedules(alg, p, c, name):
    H.load_backend(T.ORACLE_BACKEND)
    refused(T.case_inputs("er8_r16"), "score gatv2.*%s.*c = %d" % (name, c), ranks=p, alg=alg, c=c, layers=[(16, 8, 2)])


def test_gatv2_refuses_wide_heads_and_accepts_256():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    refused(case, "score gatv2.*at most 256 features, not 257", layers=[(16, 257, 1)])
    refused(case, r"hnh_attn_v2_fwd_csr_p.*include/hnh_attn_v2\.h", layers=[(16, 256, 1)])


def test_the_reference_trains():
    """The condition on the inputs of the GPU test's Adam run: the numpy reference's own loss on the planted partition falls, and every a moves."""
    pp = R.planted_partition(T.GAT_LAYERS)
    av = {k: v[0] for k, v in pp["av"].items()}
    losses, _, _, av_end = V.train(pp["rows"], pp["cols"], pp["m"], pp["x"], T.GAT_LAYERS, T.GAT_ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], av,
                                   R.LEARN_OPTIMIZER, 10, activations=("elu", "identity"))
    assert losses[-1] < losses[0] and all(np.abs(av_end[k] - av[k]).max() > 0 for k in av), losses
