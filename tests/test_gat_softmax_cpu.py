"""GAT softmax attention without a GPU: the numpy definition (tests/gat_ref.py, attention softmax) against finite differences of its forward pass,
the optional kernel group of include/hnh_attention.h (declared == bound == exported by the HIP library, disjoint from the mandatory
and grad tables, absent from the CPU test double), and the host calls on the test double: the softmax mode names the missing kernel
or the unsupported schedule, and the default mode is untouched."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_pass_ref as P
import gat_ref as R
import softmax_schedules as S
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared
from oracle import oracle as O

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
    dws, _, dx = R.backward(rows, cols, m, x, layers, alpha, g, w, attention="softmax")

    def loss(ww, xx):
        return float(np.sum(g * R.forward(rows, cols, m, xx, layers, alpha, ww, attention="softmax")))

    # LeakyReLU and ReLU are not differentiable at 0: no pre-activation may lie within +-10 steps of it (exact zeros are rows that
    # are zero whatever the perturbation: a vertex without nonzeros)
    def margin_ok(ww, xx):
        pre = R.kinks(rows, m, R.pre_activations(rows, cols, m, xx, layers, alpha, ww, attention="softmax"))
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
    txt = open(ROOT + "/include/hnh_dist.h").read()
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


# ------------------------------------------------------------------------------------------------ the kernel tests' reference and inputs
@pytest.mark.parametrize("width,scale,fsum,tol", [(7, 1.0, None, 1e-13), (100, 1.0, None, 1e-13), (5, 1.0, True, 1e-13), (16, 40.0, None, 1e-12)])
def test_extended_reference_matches_fp64(width, scale, fsum, tol):
    """attention_ld (longdouble, or math.fsum where longdouble is fp64) against the fp64 attention(); with scores up to +-1e3 the fp64
    weights exp(s - lse) carry the rounding of s (a few 1e-13), which is what the extended reference removes."""
    rng = np.random.default_rng(width)
    m = 300
    deg = rng.integers(0, 30, m)
    deg[::7] = 0
    deg[3] = 700
    rows = np.repeat(np.arange(m), deg)
    cols = rng.integers(0, m, len(rows))
    x, y = rng.uniform(-1, 1, (m, width)) * scale, rng.uniform(-1, 1, (m, width)) * scale
    perm = rng.permutation(len(rows))  # the reference takes the nonzeros in any order
    o, lse, s = P.attention(rows[perm], cols[perm], m, x, y, T.GAT_ALPHA)
    o_ld, lse_ld, s_ld = P.attention_ld(rows[perm], cols[perm], m, x, y, T.GAT_ALPHA, chunk=1000, fsum=fsum)
    assert o_ld.dtype == np.longdouble and lse_ld.dtype == np.longdouble
    assert T.rel(np.float64(o_ld), o) <= tol and T.rel(np.float64(s_ld), s) <= 1e-13
    assert np.all(np.abs(np.float64(lse_ld) - lse) <= 1e-13 * np.maximum(1.0, np.abs(lse))) and np.all(lse_ld[deg == 0] == 0)
    if scale > 1:
        assert np.abs(s).max() > 700.0


def test_max_rises():
    rowptr = np.array([0, 0, 1, 5, 9])
    s = np.array([3.0, 1.0, 2.0, 2.0, 5.0, -2.0, 0.0, 0.0, -1.0])
    got = P.max_rises(rowptr, s)
    assert [list(g) for g in got] == [[], [0], [0, 1, 3], [0, 1]]


def test_forced_schedules_rise_where_designed():
    """The designed inputs of tests/softmax_schedules.py: every row's running max rises exactly where its schedule says, and the
    schedules reach what they are for (a spike at every k <= 18, a hub row's last nonzero, every window and panel start, ties with the
    max, rises beyond exp's range)."""
    m = 4096
    rowptr, colidx, x, y, rises, group = S.build(m, 16, 3)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    assert all(np.all(np.diff(colidx[rowptr[i]:rowptr[i + 1]]) >= 0) for i in range(m)), "columns sorted within a row"
    _, _, s = P.attention(rows, colidx.astype(np.int64), m, x, y, T.GAT_ALPHA)
    got = P.max_rises(rowptr, s)
    for i in range(m):
        assert np.array_equal(got[i], rises[i]), (i, group[i], got[i], rises[i])
    g = np.array(group)
    deg = np.diff(rowptr)
    assert np.count_nonzero(deg == 0) > m // 20
    mono = np.nonzero((g == "monotone") & (deg > 0))[0]
    assert all(len(rises[i]) == deg[i] for i in mono) and deg[mono].max() >= 300
    spike = [i for i in np.nonzero(g == "spike")[0] if deg[i] > 0]
    ks = {int(rises[i][-1]) if len(rises[i]) > 1 else 0 for i in spike}
    assert set(range(19)) <= ks
    hub = [i for i in spike if deg[i] >= 600]
    assert hub and all(rises[i][-1] == deg[i] - 1 for i in hub)
    assert any(deg[i] >= 60 and rises[i][-1] >= deg[i] - 8 for i in spike), "a rise late in a row"
    for name, bounds in (("window", S.window_bounds(m, 6)), ("panel", S.panel_bounds(m, 5))):
        starts = set()
        for i in np.nonzero(g == name)[0]:
            c = colidx[rowptr[i]:rowptr[i + 1]]
            starts |= {int(np.searchsorted(bounds, c[u], side="right")) - 1 for u in rises[i]}
            assert len(rises[i]) == len(set(np.searchsorted(bounds, c, side="right")))
        assert starts == set(range(len(bounds) - 1))
        assert max(len(rises[i]) for i in np.nonzero(g == name)[0]) == len(bounds) - 1
    for i in np.nonzero((g == "ties") | (g == "tie_spike"))[0]:
        assert deg[i] == 0 or list(rises[i]) == [0]
    assert deg[(g == "ties")].max() >= 300 and len(np.unique(s[np.isin(rows, np.nonzero(g == "ties")[0])])) == 1

    def tie_spike(i):  # a score equal to the row's max right after a lower one: f == 1 at a local spike
        seg = s[rowptr[i]:rowptr[i + 1]]
        return len(seg) > 2 and np.any((seg[2:] == seg[0]) & (seg[1:-1] < seg[0]))

    tie_rows = np.nonzero(g == "tie_spike")[0]
    assert sum(tie_spike(i) for i in tie_rows) > len(tie_rows) // 2
    jumps = [np.diff(np.maximum.accumulate(s[rowptr[i]:rowptr[i + 1]]))[rises[i][1:] - 1] for i in np.nonzero(g == "jump")[0] if len(rises[i]) > 1]
    assert min(j.min() for j in jumps) > 745.0 and any(len(j) == 2 for j in jumps)


@pytest.mark.parametrize("layers,refused", [([(16, 301, 2)], True), ([(16, 514, 1)], True), ([(16, 8, 2), (16, 257, 1)], True),
                                            ([(16, 512, 1)], False), ([(16, 255, 2)], False)])
def test_softmax_names_the_width_limit(layers, refused):
    """A softmax head is one pass over its columns: f <= 512 (even) or 255 (odd).  Refused before any kernel is needed (the test
    double has none: an accepted width gets as far as naming the missing kernel)."""
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
        d = H.DistributedSparse(world, "15d_fusion2", sp, 16, 1)
        gnn = H.GAT(d, layers, T.GAT_ALPHA, attention="softmax")
        with pytest.raises(H.HnhError, match="at most 512 features" if refused else "hnh_attn_softmax_csr_p") as e:
            gnn.forwardPass()
        if refused:
            assert str(max(f for _, f, _ in layers)) in str(e.value)
        for h in (gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(1, rank))
