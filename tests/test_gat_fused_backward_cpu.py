"""The GAT's fused backward mode without a GPU: the numpy restatement of its two passes (tests/gat_pass_ref.py, over S and S^T
with the packed operand) against the definition (tests/gat_ref.py) in both attention modes, the optional kernel group of include/hnh_attn_grad.h (declared == bound
== exported by the HIP library, absent from the mandatory table and from the CPU test double), the host call, and the modes on the
test double: "fused" fails naming a kernel of the new group, an explicit "unfused" is the old pass."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, make_gat
from oracle import oracle as O

def small_problem(softmax):
    """The small ER graph of the reference's own CPU tests (32 vertices, 123 nonzeros) with T.GAT_LAYERS, plus one repeated pair."""
    rows, cols = O.erdos_renyi(5, 4)
    rows, cols = np.concatenate([rows, rows[:1]]), np.concatenate([cols, cols[:1]])
    m = 32
    x = O.dense_fill(m, T.GAT_LAYERS[0][0], 2) * T.GAT_INPUT_SCALE
    w = {(li, h): O.gat_weight(li, h, fin, fph) * (1.0 if li == 0 or softmax else 40.0)
         for li, (fin, fph, heads) in enumerate(T.GAT_LAYERS) for h in range(heads)}
    g = O.dense_fill(m, T.GAT_LAYERS[-1][1] * T.GAT_LAYERS[-1][2], 9) * 16.0
    return rows, cols, m, x, w, g


@pytest.mark.parametrize("attention", ["none", "softmax"])
def test_two_passes_equal_the_reference(attention):
    softmax = attention == "softmax"
    rows, cols, m, x, w, g = small_problem(softmax)
    want_dw, _, want_dx = R.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, attention=attention)
    got_dw, _, got_dx = R.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, attention=attention, by_passes=True)
    assert set(got_dw) == set(want_dw) and all(np.abs(v).max() > 0 for v in want_dw.values()) and np.count_nonzero(want_dx) > want_dx.size // 2
    for k in want_dw:
        assert T.rel(got_dw[k], want_dw[k]) <= T.TOL, (k, T.rel(got_dw[k], want_dw[k]))
    assert T.rel(got_dx, want_dx) <= T.TOL, T.rel(got_dx, want_dx)


@pytest.mark.parametrize("f,softmax", [(1, False), (7, True), (8, True), (33, False)])
def test_packed_layout(f, softmax):
    """[A (0) | dZ (0) | lse delta]: the dZ half and the scalars start at even columns, the width is even, the pad holds zero."""
    rng = np.random.default_rng(f)
    a, dz = rng.uniform(-1, 1, (5, f)), rng.uniform(-1, 1, (5, f))
    lse, delta = (rng.uniform(0, 1, 5), rng.uniform(-1, 1, 5)) if softmax else (None, None)
    fp = f + (f & 1)
    pw = P.fused_packed_width(f, softmax)
    assert pw == K.attn_grad_packed_width(f, softmax) == 2 * fp + (2 if softmax else 0) and pw % 2 == 0 and fp % 2 == 0
    p = P.fused_pack(a, dz, lse, delta, ld=pw + 2)
    assert np.array_equal(p[:, :f], a) and np.array_equal(p[:, fp:fp + f], dz) and np.all(np.isnan(p[:, pw:]))
    if f & 1:
        assert np.all(p[:, f] == 0.0) and np.all(p[:, fp + f] == 0.0)
    if softmax:
        assert np.array_equal(p[:, 2 * fp], lse) and np.array_equal(p[:, 2 * fp + 1], delta)


def test_attn_grad_kernels_are_an_optional_group():
    names = declared("hnh_attn_grad.h")
    assert names == {"hnh_attn_grad_row_csr_p", "hnh_attn_grad_col_csr_p", "hnh_attn_grad_pack_f64"}
    assert names == set(K.ATTN_GRAD_SIGNATURES), names ^ set(K.ATTN_GRAD_SIGNATURES)
    assert not names & declared("hnh_kernels.h") and not names & set(K.SIGNATURES), "never part of the mandatory table"
    assert not names & (set(K.GRAD_SIGNATURES) | set(K.ATTN_SIGNATURES))
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.ATTN_GRAD_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    txt = open(ROOT + "/include/hnh_attn_grad.h").read()
    assert re.search(r"#define HNH_ATTN_GRAD_MAX_F %d\b" % K.ATTN_GRAD_MAX_F, txt)
    assert C.sizeof(K.AttnGrad) == 96  # struct hnh_attn_grad: ten pointers and pitches, two ints, one double


def test_host_call_declared_and_exported():
    assert "hnh_gat_set_backward" in declared("hnh_dist.h") and "hnh_gat_set_backward" in H.SIGNATURES
    txt = open(ROOT + "/include/hnh_dist.h").read()
    assert re.search(r"#define HNH_GAT_BACKWARD_UNFUSED 0\b", txt) and re.search(r"#define HNH_GAT_BACKWARD_FUSED 1\b", txt)
    assert hasattr(H.lib(), "hnh_gat_set_backward")
    assert H.GAT.BACKWARD == {"unfused": 0, "fused": 1}


def test_fused_on_the_test_double_names_the_missing_kernel():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, backward="fused")
        g = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.forwardPass()
        with pytest.raises(H.HnhError, match=r"backwardPass.*hnh_attn_grad_row_csr_p.*include/hnh_attn_grad\.h"):
            gnn.backwardPass(g)
        with pytest.raises(ValueError):
            gnn.set_backward("half-fused")
        assert H.lib().hnh_gat_set_backward(gnn.h, 7) != 0, "an unknown mode number is refused by the C ABI too"
        gnn.set_backward("unfused")  # no new forward pass: the old pass's own complaint, about a kernel of include/hnh_grad.h
        with pytest.raises(H.HnhError, match=r"hnh_gemm_tn_f64.*include/hnh_grad\.h"):
            gnn.backwardPass(g)
        gnn.set_backward("fused")
        gnn.forwardPass()  # the process and the operator live on
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (g, out, gnn, d, sp):
            h.free()
        return res

    per_rank = H.run_spmd(2, rank)
    assert all(np.isfinite(r).all() for r in per_rank)


def test_explicit_unfused_is_the_default_pass():
    """On the double both fail in the same place, with the same words."""
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        msgs = []
        for kw in ({}, {"backward": "unfused"}):
            sp, d, gnn = make_gat(world, case, "15d_fusion1", 1, **kw)
            g = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
            gnn.forwardPass()
            with pytest.raises(H.HnhError, match=r"include/hnh_grad\.h") as e:
                gnn.backwardPass(g)
            msgs.append(str(e.value))
            for h in (g, gnn, d, sp):
                h.free()
        return msgs

    for msgs in H.run_spmd(2, rank):
        assert msgs[0] == msgs[1] and "hnh_gemm_tn_f64" in msgs[0] and "hnh_attn_grad" not in msgs[0]


@pytest.mark.parametrize("alg,p,c", [("15d_fusion1", 4, 2), ("15d_fusion2", 4, 2), ("15d_sparse", 2, 1), ("25d_dense_replicate", 4, 1)])
def test_fused_refuses_unsupported_schedules(alg, p, c):
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, alg, c, layers=[(16, 8, 2)], backward="fused")
        g = H.Dense.create(world, *gnn.buffer_shape(1))
        with pytest.raises(H.HnhError, match="backwardPass"):
            gnn.backwardPass(g)
        for h in (g, gnn, d, sp):
            h.free()
        return True

    assert all(H.run_spmd(p, rank))
