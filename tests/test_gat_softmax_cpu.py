"""GAT softmax attention without a GPU: the numpy definition (tests/gat_softmax_ref.py) against finite differences of its forward pass,
the optional kernel group of include/hnh_attention.h (declared == bound == exported by the HIP library, disjoint from the mandatory
and grad tables, absent from the CPU test double), and the host calls on the test double: the softmax mode names the missing kernel
or the unsupported schedule, and the default mode is untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gat_softmax_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(hnh_[a-z0-9_]+)\s*\(", txt))


def fd_problem():
    """A small ER graph (32 vertices, 123 nonzeros) with T.GAT_LAYERS and weights of the usual 1/sqrt(fan-in) scale in BOTH layers:
    the softmax keeps the second layer's inputs of order one, no hand-tuned scale is needed."""
    rows, cols = O.erdos_renyi(5, 4)
    m = 32
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, (m, T.GAT_LAYERS[0][0]))
    w = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(T.GAT_LAYERS) for h in range(heads)}
    g = O.dense_fill(m, T.GAT_LAYERS[-1][1] * T.GAT_LAYERS[-1][2], 9) * 16.0  # dL/d(out) of L = <g, out>
    return rows, cols, m, x, w, g


def test_reference_backward_matches_finite_differences():
    rows, cols, m, x, w, g = fd_problem()
    layers, alpha, step = T.GAT_LAYERS, T.GAT_ALPHA, 1e-6
    dws, dx = R.backward(rows, cols, m, x, layers, alpha, g, w)

    def loss(ww, xx):
        return float(np.sum(g * R.forward(rows, cols, m, xx, layers, alpha, ww)))

    # LeakyReLU and ReLU are not differentiable at 0: no pre-activation may lie within +-10 steps of it (exact zeros are rows that
    # are zero whatever the perturbation: a vertex without nonzeros)
    def margin_ok(ww, xx):
        pre = R.pre_activations(rows, cols, m, xx, layers, alpha, ww)
        return np.abs(pre[pre != 0]).min() > 10 * step

    assert margin_ok(w, x)
    rng = np.random.default_rng(3)
    for key, wk in w.items():
        probes = [(0, 0), (wk.shape[0] - 1, wk.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in wk.shape) for _ in range(3)]
        fd, an = [], []
        for p, q in probes:
            plus, minus = dict(w), dict(w)
            plus[key], minus[key] = wk.copy(), wk.copy()
            plus[key][p, q] += step
            minus[key][p, q] -= step
            assert margin_ok(plus, x) and margin_ok(minus, x)
            fd.append((loss(plus, x) - loss(minus, x)) / (2 * step))
            an.append(dws[key][p, q])
        err = np.max(np.abs(np.subtract(fd, an))) / np.max(np.abs(an))
        assert err <= 1e-6, (key, err)
    fd, an = [], []
    for p, q in [(0, 0), (m - 1, x.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in x.shape) for _ in range(4)]:
        xp, xm = x.copy(), x.copy()
        xp[p, q] += step
        xm[p, q] -= step
        assert margin_ok(w, xp) and margin_ok(w, xm)
        fd.append((loss(w, xp) - loss(w, xm)) / (2 * step))
        an.append(dx[p, q])
    err = np.max(np.abs(np.subtract(fd, an))) / np.max(np.abs(an))
    assert err <= 1e-6, err
    assert np.count_nonzero(dx) > dx.size // 2 and all(np.abs(d).max() > 0 for d in dws.values()), "the gradients must not be vacuous"


def test_reference_forward_is_a_row_softmax():
    """Each non-empty row's weights sum to 1 (so o is a convex combination of the A_j), even with scores far beyond exp's range."""
    rows, cols = O.erdos_renyi(6, 8)
    m = 64
    s = np.random.default_rng(1).uniform(-1e3, 1e3, len(rows))
    a, lse = R.row_softmax(rows, m, s)
    sums = np.bincount(rows, weights=a, minlength=m)
    live = np.bincount(rows, minlength=m) > 0
    assert np.all(np.isfinite(a)) and np.allclose(sums[live], 1.0, rtol=0, atol=1e-13) and np.all(lse[~live] == 0.0)


def test_attention_kernels_are_an_optional_group():
    names = declared("hnh_attention.h")
    assert names and names == set(K.ATTN_SIGNATURES), names ^ set(K.ATTN_SIGNATURES)
    assert not names & declared("hnh_kernels.h") and not names & declared("hnh_grad.h"), "declared in hnh_attention.h only"
    assert not names & set(K.SIGNATURES) and not names & set(K.GRAD_SIGNATURES), "never part of the mandatory or grad tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.ATTN_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works


def test_host_call_declared():
    assert "hnh_gat_set_attention" in declared("hnh_dist.h") and "hnh_gat_set_attention" in H.SIGNATURES
    txt = open(os.path.join(ROOT, "include", "hnh_dist.h")).read()
    assert re.search(r"#define HNH_GAT_ATTENTION_NONE 0\b", txt) and re.search(r"#define HNH_GAT_ATTENTION_SOFTMAX 1\b", txt)


def gat_output(world, case, alg, c, make):
    sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
    d = H.DistributedSparse(world, alg, sp, case["R"], c)
    gnn = make(d)
    for li, (fin, fph, heads) in enumerate(T.GAT_LAYERS):
        for h in range(heads):
            gnn.set_weight(li, h, O.gat_weight(li, h, fin, fph))
    d.setRValue(T.GAT_LAYERS[0][0])
    x = H.Dense.create(world, *gnn.buffer_shape(0))
    x.upload(T.fill_local(d.submatrices(H.BMAT), x.shape, case["A"] * T.GAT_INPUT_SCALE))
    gnn.set_input(x)
    gnn.forwardPass()
    out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
    gnn.get_output(out)
    res = out.download()
    for h in (x, out, gnn, d, sp):
        h.free()
    return res


def test_explicit_none_is_the_old_gat():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")
    for alg, p, c in (("15d_fusion2", 2, 1), ("15d_fusion1", 2, 1)):
        old = H.run_spmd(p, lambda wd: gat_output(wd, case, alg, c, lambda d: H.GAT(d, T.GAT_LAYERS, T.GAT_ALPHA)))
        new = H.run_spmd(p, lambda wd: gat_output(wd, case, alg, c, lambda d: H.GAT(d, T.GAT_LAYERS, T.GAT_ALPHA, attention="none")))
        assert all(np.array_equal(a, b) for a, b in zip(old, new)) and any(np.count_nonzero(a) for a in old)


def test_softmax_on_the_test_double_names_the_missing_kernel():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
        d = H.DistributedSparse(world, "15d_fusion2", sp, case["R"], 1)
        gnn = H.GAT(d, T.GAT_LAYERS, T.GAT_ALPHA, attention="softmax")
        with pytest.raises(H.HnhError, match="hnh_attn_softmax_csr_p"):
            gnn.forwardPass()
        with pytest.raises(ValueError):
            gnn.set_attention("sparsemax")
        gnn.set_attention("none")  # the process and the operator live on
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, gnn, d, sp):
            h.free()
        return res

    per_rank = H.run_spmd(2, rank)
    assert all(np.isfinite(r).all() for r in per_rank)


SCHEDULE_NAMES = {"15d_sparse": "1.5D Sparse Shifting", "25d_dense_replicate": "2.5D Cannon's Algorithm Replicating Dense",
                  "25d_sparse_replicate": "2.5D Cannon's Algorithm Replicating Sparse"}


@pytest.mark.parametrize("alg,p,c", [("15d_fusion1", 2, 1), ("15d_fusion1", 4, 2), ("15d_sparse", 2, 1), ("25d_dense_replicate", 4, 1),
                                     ("25d_sparse_replicate", 4, 1), ("15d_fusion2", 4, 2)])
def test_softmax_refuses_unsupported_schedules(alg, p, c):
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
        d = H.DistributedSparse(world, alg, sp, 16, c)
        gnn = H.GAT(d, [(16, 8, 2)], T.GAT_ALPHA, attention="softmax")
        with pytest.raises(H.HnhError, match="softmax.*%s.*c = %d" % (SCHEDULE_NAMES.get(alg, alg), c)):
            gnn.forwardPass()
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(p, rank))
