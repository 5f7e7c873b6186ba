"""The GAT's additive (a1, a2) attention score without a GPU: the numpy definition (tests/gat_ref.py with score "additive"; the
packed layouts and the passes as the kernels take them: tests/gat_pass_ref.py) against central finite differences, the optional kernel
group of include/hnh_attn_additive.h (declared == bound == exported by the HIP library, disjoint from the four existing tables, absent from the
CPU test double), the host calls, and on the test double: score "additive" names a kernel of the new group and its header, every
unsupported shape is refused by name, and score "dot" on the same object runs as before."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat
from oracle import oracle as O

MODE = dict(attention="softmax", score="additive")
GROUP = {"hnh_attn_add_fwd_csr_p", "hnh_attn_add_row_csr_p", "hnh_attn_add_col_csr_p", "hnh_attn_add_scores_f64", "hnh_attn_add_pack_f64",
         "hnh_attn_add_update_f64"}


def test_reference_backward_matches_finite_differences():
    rows, cols, m, x, w, av, g = fd_problem()
    layers, alpha, step = T.GAT_LAYERS, T.GAT_ALPHA, 1e-6
    dws, das, dx = R.backward(rows, cols, m, x, layers, alpha, g, w, av, **MODE)

    def loss(ww, aa, xx):
        return float(np.sum(g * R.forward(rows, cols, m, xx, layers, alpha, ww, aa, **MODE)))

    # LeakyReLU and ReLU are not differentiable at 0: every LeakyReLU input z and every ReLU input o of a non-empty row is at least
    # 100 steps away from it (exact zeros are rows that are zero whatever the perturbation: a vertex without nonzeros)
    def margin_ok(ww, aa, xx, steps=100):
        pre = R.kinks(rows, m, R.pre_activations(rows, cols, m, xx, layers, alpha, ww, aa, **MODE))
        return np.abs(pre[pre != 0]).min() >= steps * step

    assert margin_ok(w, av, x)
    assert all(np.all(a != 0) and np.all(b != 0) for a, b in das.values()), "every entry of da1, da2 is non-zero"
    assert np.count_nonzero(dx) > dx.size // 2 and all(np.abs(d).max() > 0 for d in dws.values()), "the gradients must not be vacuous"

    def fd_of(perturb, probes):
        out = []
        for idx in probes:
            plus, minus = perturb(idx, step), perturb(idx, -step)
            assert margin_ok(*plus, steps=99) and margin_ok(*minus, steps=99)
            out.append((loss(*plus) - loss(*minus)) / (2 * step))
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
    for key, (a1, a2) in av.items():  # every entry of every da1, da2
        for which in (0, 1):
            def perturb(idx, h, key=key, which=which):
                aa = dict(av)
                pair = [av[key][0].copy(), av[key][1].copy()]
                pair[which][idx] += h
                aa[key] = tuple(pair)
                return w, aa, x

            probes = list(range(len(a1)))
            an = das[key][which]
            err = np.max(np.abs(fd_of(perturb, probes) - an)) / np.max(np.abs(an))
            assert err <= 1e-6, (key, which, err)
    probes = [(0, 0), (m - 1, x.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in x.shape) for _ in range(4)]

    def perturb_x(idx, h):
        xx = x.copy()
        xx[idx] += h
        return w, av, xx

    an = np.array([dx[idx] for idx in probes])
    err = np.max(np.abs(fd_of(perturb_x, probes) - an)) / np.max(np.abs(an))
    assert err <= 1e-6, err


def test_two_passes_with_the_packed_operands_equal_the_definition():
    rows, cols, m, x, w, av, g = fd_problem()
    want = R.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, av, **MODE)
    got = R.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, av, by_passes=True, **MODE)
    for k in want[0]:
        assert T.rel(got[0][k], want[0][k]) <= T.TOL
        assert T.rel(got[1][k][0], want[1][k][0]) <= T.TOL and T.rel(got[1][k][1], want[1][k][1]) <= T.TOL
    assert T.rel(got[2], want[2]) <= T.TOL
    # the forward pass as the kernel takes it, and its extended-precision twin
    fin, f, _ = T.GAT_LAYERS[0]
    a_mat = x @ w[(0, 0)]
    mm = P.scored(a_mat, *av[(0, 0)])
    o, lse, z, _ = P.fwd_pass(rows, cols, m, mm, mm, f, T.GAT_ALPHA)
    _, trace = R.forward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, w, av, keep_trace=True, **MODE)
    assert T.rel(o, trace[0][3][0][3]) <= T.TOL and T.rel(lse, trace[0][3][0][4]) <= T.TOL
    o_ld, lse_ld = P.fwd_pass_ld(rows, cols, m, mm, mm, f, T.GAT_ALPHA)
    assert o_ld.dtype == np.longdouble and T.rel(np.float64(o_ld), o) <= 1e-13 and T.rel(np.float64(lse_ld), lse) <= 1e-13


def test_forward_is_finite_far_outside_exps_range():
    rows, cols = O.erdos_renyi(6, 8)
    m, f = 64, 6
    rng = np.random.default_rng(1)
    a_mat = rng.uniform(-1, 1, (m, f))
    mm = P.scored(a_mat, rng.uniform(-1, 1, f) * 400, rng.uniform(-1, 1, f) * 400)
    o, lse, z, _ = P.fwd_pass(rows, cols, m, mm, mm, f, T.GAT_ALPHA)
    assert np.abs(z).max() > 800 and np.all(np.isfinite(o)) and np.all(np.isfinite(lse))


@pytest.mark.parametrize("f", [1, 2, 7, 8, 33])
def test_packed_layouts(f):
    """[A (0) | s t] and [dZ (0) | s lse delta 0]: the scalars start at an even column, the widths are even, the pads hold zero."""
    rng = np.random.default_rng(f)
    a, dz = rng.uniform(-1, 1, (5, f)), rng.uniform(-1, 1, (5, f))
    a1, a2 = rng.uniform(-1, 1, f), rng.uniform(-1, 1, f)
    lse, delta = rng.uniform(0, 1, 5), rng.uniform(-1, 1, 5)
    fp = f + (f & 1)
    assert P.scored_width(f) == K.attn_add_scored_width(f) == fp + 2 and P.packed_width(f) == K.attn_add_packed_width(f) == fp + 4
    mm = P.scored(a, a1, a2, ld=fp + 4)
    assert np.array_equal(mm[:, :f], a) and np.array_equal(mm[:, fp], a @ a1) and np.array_equal(mm[:, fp + 1], a @ a2)
    assert np.all(np.isnan(mm[:, fp + 2:]))
    q = P.pack(dz, mm[:, fp], lse, delta, ld=fp + 6)
    assert np.array_equal(q[:, :f], dz) and np.array_equal(q[:, fp], mm[:, fp]) and np.array_equal(q[:, fp + 1], lse)
    assert np.array_equal(q[:, fp + 2], delta) and np.all(q[:, fp + 3] == 0.0) and np.all(np.isnan(q[:, fp + 4:]))
    if f & 1:
        assert np.all(mm[:, f] == 0.0) and np.all(q[:, f] == 0.0)
    txt = open(ROOT + "/include/hnh_attn_additive.h").read()
    assert re.search(r"#define HNH_ATTN_ADD_MAX_F %d\b" % K.ATTN_ADD_MAX_F, txt)


def test_additive_kernels_are_an_optional_group():
    names = declared("hnh_attn_additive.h")
    assert names == GROUP
    assert names == set(K.ATTN_ADD_SIGNATURES), names ^ set(K.ATTN_ADD_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES):
        assert not names & set(table), "disjoint from the four existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.ATTN_ADD_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.AttnAdd) == 144  # struct hnh_attn_add: sixteen pointers and pitches, an int (padded), a double


def test_host_calls_declared_and_exported():
    for n in ("hnh_gat_set_score", "hnh_gat_set_attn_vectors", "hnh_gat_get_attn_grads"):
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n), n
    txt = open(ROOT + "/include/hnh_dist.h").read()
    assert re.search(r"#define HNH_GAT_SCORE_DOT 0\b", txt) and re.search(r"#define HNH_GAT_SCORE_ADDITIVE 1\b", txt)
    assert H.GAT.SCORE == {"dot": 0, "additive": 1}


def test_additive_on_the_test_double_names_the_missing_kernel():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, attention="softmax", score="additive")
        f = T.GAT_LAYERS[0][1]
        gnn.set_attention_vectors(0, 1, np.ones(f), -np.ones(f))
        with pytest.raises(H.HnhError, match=r"additive.*hnh_attn_add_[a-z0-9_]+.*include/hnh_attn_additive\.h") as e:
            gnn.forwardPass()
        assert re.search(r"hnh_attn_add_[a-z0-9_]+", str(e.value)).group(0) in GROUP
        with pytest.raises(ValueError):
            gnn.set_score("bilinear")
        assert H.lib().hnh_gat_set_score(gnn.h, 7) != 0, "an unknown score number is refused by the C ABI too"
        with pytest.raises(H.HnhError, match="attention-vector gradient"):
            gnn.attention_grad(0, 0)
        gnn.set_score("dot")  # the process and the operator live on: the dot-product GAT on the same object
        gnn.set_attention("none")
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, gnn, d, sp):
            h.free()
        return res

    def plain(world):  # a GAT that never heard of the score
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1)
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, gnn, d, sp):
            h.free()
        return res

    per_rank, want = H.run_spmd(2, rank), H.run_spmd(2, plain)
    assert all(np.isfinite(r).all() for r in per_rank) and all(np.array_equal(a, b) for a, b in zip(per_rank, want))


SCHEDULE_NAMES = {"15d_sparse": "1.5D Sparse Shifting", "25d_dense_replicate": "2.5D Cannon's Algorithm Replicating Dense",
                  "15d_fusion1": "15d_fusion1", "15d_fusion2": "15d_fusion2"}


@pytest.mark.parametrize("alg,p,c", [("15d_fusion1", 4, 2), ("15d_fusion2", 4, 2), ("15d_sparse", 2, 1), ("25d_dense_replicate", 4, 1)])
def test_additive_refuses_unsupported_schedules(alg, p, c):
    """The four shapes of test_fused_refuses_unsupported_schedules: forward and backward name the schedule and c."""
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, alg, c, layers=[(16, 8, 2)], attention="softmax", score="additive")
        g = H.Dense.create(world, *gnn.buffer_shape(1))
        words = "score additive.*%s.*c = %d" % (SCHEDULE_NAMES[alg], c)
        with pytest.raises(H.HnhError, match=words):
            gnn.forwardPass()
        with pytest.raises(H.HnhError, match=words):
            gnn.backwardPass(g)
        for h in (g, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(p, rank))


@pytest.mark.parametrize("layers,attention,words", [([(16, 8, 2)], "none", "score additive.*attention mode softmax only.*attention mode none"),
                                                    ([(16, 257, 1)], "softmax", "score additive.*at most 256 features, not 257"),
                                                    ([(16, 8, 2), (16, 300, 1)], "softmax", "score additive.*at most 256 features, not 300")])
def test_additive_refuses_attention_none_and_wide_heads(layers, attention, words):
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, layers=layers, attention=attention, score="additive")
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        with pytest.raises(H.HnhError, match=words):
            gnn.forwardPass()
        with pytest.raises(H.HnhError, match=words):
            gnn.backwardPass(g)
        for h in (g, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(1, rank))


def test_a_256_feature_head_is_accepted_as_far_as_the_kernels():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, layers=[(16, 256, 1)], attention="softmax", score="additive")
        with pytest.raises(H.HnhError, match=r"hnh_attn_add_fwd_csr_p.*include/hnh_attn_additive\.h"):
            gnn.forwardPass()
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(1, rank))


def test_the_reference_trains():
    """The condition on the inputs of the GPU test's SGD: with this step size the numpy reference's own loss falls at every step, and
    every a1, a2 moves."""
    case = T.case_inputs("er8_r16")
    rows, cols, m = case["rows"], case["cols"], case["M"]
    x = case["A"] * T.GAT_INPUT_SCALE
    layers = T.GAT_LAYERS
    target = O.dense_fill(m, layers[-1][1] * layers[-1][2], 21) * R.SGD_TARGET_SCALE
    w = {(li, h): O.gat_weight(li, h, fin, fph) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    av = R.vectors_of(layers)
    losses, av_end = R.descend(rows, cols, m, x, layers, T.GAT_ALPHA, target, w, av, **MODE)
    assert len(losses) == R.SGD_STEPS + 1 and all(losses[i + 1] < losses[i] for i in range(R.SGD_STEPS)), losses
    assert all(np.abs(av_end[k][i] - av[k][i]).max() > 0 for k in av for i in (0, 1))
