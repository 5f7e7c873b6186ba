"""GAT backward pass without a GPU: the numpy definition (tests/gat_ref.py, attention none) against finite differences of the forward pass,
the optional kernel group of include/hnh_grad.h (declared == bound == exported by the HIP library, absent from the mandatory table),
and the host calls, which on the CPU test double (no such kernels) fail with an error naming the missing one."""
import ctypes as C
import numpy as np
import pytest

import gat_cpu_harness as CH
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from oracle import oracle as O

def fd_problem():
    """A small ER graph (32 vertices, 123 nonzeros) with T.GAT_LAYERS; the second layer's weights are scaled up so that its
    pre-activations are of order one, like the first layer's."""
    rows, cols = O.erdos_renyi(5, 4)
    m = 32
    x = O.dense_fill(m, T.GAT_LAYERS[0][0], 2) * T.GAT_INPUT_SCALE
    w = {(li, h): O.gat_weight(li, h, fin, fph) * (1.0 if li == 0 else 40.0)
         for li, (fin, fph, heads) in enumerate(T.GAT_LAYERS) for h in range(heads)}
    g = O.dense_fill(m, T.GAT_LAYERS[-1][1] * T.GAT_LAYERS[-1][2], 9) * 16.0  # dL/d(out) of L = <g, out>
    return rows, cols, m, x, w, g


def test_reference_backward_matches_finite_differences():
    rows, cols, m, x, w, g = fd_problem()
    layers, alpha, step = T.GAT_LAYERS, T.GAT_ALPHA, 1e-6
    dws, _, dx = R.backward(rows, cols, m, x, layers, alpha, g, w)

    def loss(ww, xx):
        return float(np.sum(g * R.forward(rows, cols, m, xx, layers, alpha, ww)))

    # LeakyReLU and ReLU are not differentiable at 0: no pre-activation may lie within +-10 steps of it (exact zeros are rows that
    # are zero whatever the perturbation: a vertex without nonzeros, or an output row that ReLU cleared)
    def margin_ok(ww, xx):
        pre = R.kinks(rows, m, R.pre_activations(rows, cols, m, xx, layers, alpha, ww))
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
    # ... and the definition is the recorded one, on the problem the recorded results were computed for
    rows, cols, m, x, w, _, g = CH.fd_problem()
    assert CH.pinned_error("none_dot", R.forward(rows, cols, m, x, layers, alpha, w), *R.backward(rows, cols, m, x, layers, alpha, g, w)) <= 1e-13


def test_grad_kernels_are_an_optional_group():
    names = CH.declared("hnh_grad.h")
    assert names and names == set(K.GRAD_SIGNATURES), names ^ set(K.GRAD_SIGNATURES)
    assert not names & CH.declared("hnh_kernels.h") and not names & set(K.SIGNATURES), "never part of the mandatory table"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.GRAD_SIGNATURES[n][1]
    assert lib.hnh_gemm_tn_f64_workspace(1024, 1024, 1 << 18) == 8 * 1024 * 1024  # eight slices of K = 2^15 for 64 tiles
    assert lib.hnh_gemm_tn_f64_workspace(16, 8, 1) == 0
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works


def test_host_calls_declared():
    names = CH.declared("hnh_dist.h")
    for n in ("hnh_gat_backward", "hnh_gat_get_weight_grad", "hnh_gat_get_input_grad"):
        assert n in names and n in H.SIGNATURES


def test_backward_on_the_test_double_names_the_missing_kernel():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
        d = H.DistributedSparse(world, "15d_fusion1", sp, case["R"], 1)
        gnn = H.GAT(d, T.GAT_LAYERS, T.GAT_ALPHA)
        g = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.forwardPass()
        with pytest.raises(H.HnhError, match="hnh_gemm_tn_f64"):
            gnn.backwardPass(g)
        with pytest.raises(H.HnhError):
            gnn.weight_grad(0, 0)
        gnn.forwardPass()  # the process and the operator live on
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (g, out, gnn, d, sp):
            h.free()
        return res

    per_rank = H.run_spmd(2, rank)
    assert all(np.isfinite(r).all() for r in per_rank)
