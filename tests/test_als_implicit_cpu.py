"""Implicit-feedback ALS with confidence weights without a GPU (api.ImplicitALS, csrc/host/als_implicit.hpp, include/hnh_als_implicit.h;
tests/als_implicit_ref.py is the definition).

The definition: against an independent dense solve of (G + Y_i^T diag(w) Y_i + lambda I) x = rhs per row after R iterations (CG is exact
after R steps of an R x R system, up to rounding on systems this well conditioned: bound 1e-13, observed 2.2e-15) and unchanged after 4 R
(the guarded update does not run away from a converged row); float64 against long double (a half-step: 1e-13, observed 2.3e-15; the
operator tests' protocol of four unconverged half-steps: a tenth of T.TOL, observed 4.0e-13 at R = 128); the closed form of the loss
against the sum over the whole M x N grid (1e-14: a pairwise sum of 2.3 million non-negative terms rounds log2(n) eps = 2.4e-15; observed
5.9e-16); every half-step of three alternating steps lowers the loss by at least 0.5 % (observed ratios 0.76 .. 0.988); a row with
rs == 0 is frozen bit for bit and there is no NaN.
The optional kernel group: declared == bound == exported by the HIP library, absent from both CPU test doubles.
The refusals, by name.  On the second test double with loopback ranks, composed mode runs the whole path under the stream-order checker:
factors, Gram matrices and losses within T.TOL of the definition, every rank the same losses, 0 races, and a DistributedALS beside it
returns the bits it returned alone."""
import ctypes as C
import os

import numpy as np
import pytest

import als_common
import als_implicit_common as IC
import als_implicit_ref as IR
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared

GROUP = {"hnh_gram_rows_f64"}
HOST_CALLS = ("hnh_ials_create", "hnh_ials_destroy", "hnh_ials_set_confidence", "hnh_ials_initialize_embeddings", "hnh_ials_set_embeddings",
              "hnh_ials_get_embeddings", "hnh_ials_half_step", "hnh_ials_run", "hnh_ials_loss", "hnh_ials_gram", "hnh_ials_set_folded")
OPERATOR_CASES = [("hub", R, p, c) for R in (8, 17, 100) for p, c in ((1, 1), (4, 1), (5, 1), (4, 2))] + [("rmat", 8, 1, 1)]


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("g,R", [("hub", 8), ("hub", 17), ("rmat", 8)])
def test_definition_meets_the_dense_solve_and_stays_there(g, R):
    c = IR.inputs(g, R)
    for rows, cols, x, y in ((c["rows"], c["cols"], c["A"], c["B"]), (c["cols"], c["rows"], c["B"], c["A"])):
        want = IR.dense_solve(rows, cols, c["w"], y, IR.LAMBDA, x.shape[0])
        once = IR.half_step(rows, cols, c["w"], x, y, IR.LAMBDA, R)
        later = IR.half_step(rows, cols, c["w"], x, y, IR.LAMBDA, 4 * R)
        print("observed against the dense solve: %.2e after R iterations, %.2e after 4 R" % (T.rel(once, want), T.rel(later, want)))
        assert T.rel(once, want) <= 1e-13 and T.rel(later, want) <= 1e-13
        assert np.all(np.isfinite(later))


@pytest.mark.parametrize("R", [8, 17, 100, 128])
def test_float64_is_a_good_enough_model(R):
    """A half-step of either factor from the case's inputs in float64 against long double: 1e-13.  The operator tests run FOUR half-steps
    of two (unconverged) iterations, each starting from the last one's rounded result, and hold the operator to T.TOL: for that protocol
    the model's own rounding may take a tenth of it, as tests/als_common.py allows the ALS model."""
    c = IR.inputs("hub", R)
    worst = 0.0
    for rows, cols, x, y in ((c["rows"], c["cols"], c["A"], c["B"]), (c["cols"], c["rows"], c["B"], c["A"])):
        exact = IR.half_step(rows, cols, c["w"], x, y, IR.LAMBDA, IC.ITERS, np.longdouble)
        worst = max(worst, float(T.rel(IR.half_step(rows, cols, c["w"], x, y, IR.LAMBDA, IC.ITERS), exact)))
    a, b, losses = IR.run(c["rows"], c["cols"], c["w"], c["A"], c["B"], IR.LAMBDA, IC.STEPS, IC.ITERS, np.longdouble)
    want = IR.expected("hub", R)
    protocol = float(max(T.rel(want["A"], a), T.rel(want["B"], b), T.rel(want["losses"], losses)))
    print("observed float64 against long double at R = %d: half-step %.2e, the operator tests' protocol %.2e" % (R, worst, protocol))
    assert worst <= 1e-13
    assert protocol <= T.TOL / 10


@pytest.mark.parametrize("g", ["hub", "rmat"])
def test_closed_form_of_the_loss_is_the_sum_over_all_pairs(g):
    c = IR.inputs(g, 8)
    closed = IR.loss(c["rows"], c["cols"], c["w"], c["A"], c["B"], IR.LAMBDA)
    grid = IR.loss_grid(c["rows"], c["cols"], c["w"], c["A"], c["B"], IR.LAMBDA, c["M"], c["N"])
    print("observed closed form against the grid: %.2e" % (abs(closed - grid) / grid))
    assert abs(closed - grid) <= 1e-14 * grid


def test_every_half_step_lowers_the_loss():
    c = IR.inputs("hub", 8)
    _, _, losses = IR.run(c["rows"], c["cols"], c["w"], c["A"], c["B"], IR.LAMBDA, 3, 3)
    ratios = losses[1:] / losses[:-1]
    print("observed loss ratios:", ratios)
    assert len(ratios) == 6 and np.all(ratios <= 0.995)


def test_a_row_without_residual_is_frozen():
    c = IR.inputs("hub", 8)
    assert not np.any(c["rows"] == 7), "row 7 of hub is empty"
    x = c["A"].copy()
    x[7] = 0.0  # an empty row at zero: rhs = 0 and M(0) = 0, so rs == 0 from the start
    x[1] = IR.dense_solve(c["rows"], c["cols"], c["w"], c["B"], IR.LAMBDA, c["M"])[1]  # a hub row at its solution: rs is rounding
    got = IR.half_step(c["rows"], c["cols"], c["w"], x, c["B"], IR.LAMBDA, 16)
    assert np.all(np.isfinite(got))
    assert got[7].tobytes() == x[7].tobytes()
    assert T.rel(got[1], x[1]) <= 1e-13


# ------------------------------------------------------------------------------------------------ the group and the host calls
def test_gram_rows_is_an_optional_group():
    names = declared("hnh_als_implicit.h")
    assert names == GROUP == set(K.ALS_IMPLICIT_SIGNATURES)
    for header in [h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h") and h != "hnh_als_implicit.h"]:
        assert not names & declared(header), header
    for table in [n for n in dir(K) if n.endswith("SIGNATURES") and n != "ALS_IMPLICIT_SIGNATURES"]:
        assert not names & set(getattr(K, table)), table
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.ALS_IMPLICIT_SIGNATURES[n][1] and getattr(lib, n).restype == K.ALS_IMPLICIT_SIGNATURES[n][0]
    for path in (T.ORACLE_BACKEND, T.ORACLE_GAT_BACKEND):
        dbl = C.CDLL(path)
        for n in names:
            assert not hasattr(dbl, n), "the CPU test double %s does not export %s" % (os.path.basename(path), n)
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.GramCg) == 32 and K.GRAM_MAX_R == 256
    assert "#define HNH_GRAM_MAX_R 256" in open(os.path.join(ROOT, "include", "hnh_als_implicit.h")).read()


def test_host_calls_declared_and_exported():
    for n in HOST_CALLS:
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n), n
    for name in ("set_confidence", "initializeEmbeddings", "set_embeddings", "get_embeddings", "half_step", "run", "loss", "gram", "set_folded"):
        assert callable(getattr(H.ImplicitALS, name))


# ------------------------------------------------------------------------------------------------ on the test doubles
@pytest.fixture
def gat_double():
    assert H.load_backend(T.ORACLE_GAT_BACKEND) == "oracle-cpu-test-double-gat"
    lib = C.CDLL(T.ORACLE_GAT_BACKEND)
    lib.hnh_oracle_order_report.restype = C.c_long
    lib.hnh_oracle_order_accesses.restype = C.c_long
    lib.hnh_oracle_order_enable(1)
    yield lib
    H.load_backend(T.ORACLE_BACKEND)  # the modules after this one find the plain double, as before


def drain(lib):
    buf = C.create_string_buffer(16384)
    return lib.hnh_oracle_order_report(buf, 16384), buf.value.decode()


def small_case():
    return IR.inputs("rmat", 8)


def test_refusals_on_the_second_test_double(gat_double):
    case = small_case()

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], case["vals"])
        for alg, p, c, R in (("15d_fusion1", 1, 1, 8), ("15d_sparse", 1, 1, 8), ("25d_dense_replicate", 1, 1, 8), ("25d_sparse_replicate", 1, 1, 8)):
            d = H.DistributedSparse(world, alg, sp, R, c)
            with pytest.raises(H.HnhError, match="Implicit_ALS supports the schedule 15d_fusion2 only, not .*(15d_fusion1|1.5D|2.5D)"):
                H.ImplicitALS(d, 0.1)
            d.free()
        d = H.DistributedSparse(world, "15d_fusion2", sp, 8, 1)
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            with pytest.raises(H.HnhError, match="finite lambda > 0"):
                H.ImplicitALS(d, bad)
        s = IC.Solver(world, 1, case, False)
        s.set(case["A"], case["B"])
        for value in (-1e-300, float("nan"), float("inf")):
            for side, like in ((0, s.d.like_S_values), (1, s.d.like_ST_values)):
                w = like(1.0)
                host = w.download()
                host[len(host) // 2] = value
                w.upload(host)
                with pytest.raises(H.HnhError, match="finite weights >= 0"):
                    s.als.set_confidence(*((w, s.ws[1]) if side == 0 else (s.ws[0], w)))
                w.free()
        short = H.Vec.create(world, 3)
        with pytest.raises(H.HnhError, match="wrong length"):
            s.als.set_confidence(short, s.ws[1])
        short.free()
        before = s.als.loss()
        s.als.set_folded(True)
        with pytest.raises(H.HnhError, match=r"Implicit_ALS in folded mode needs the kernel hnh_gram_rows_f64.*liboracle_backend_gat\.so.*include/hnh_als_implicit\.h"):
            s.als.half_step(H.AMAT, 1)
        a, b = s.get()
        assert np.array_equal(a, T.fill_local(s.subA, a.shape, case["A"])) and s.als.loss() == before, "refused before anything ran"
        s.als.set_folded(False)
        s.als.half_step(H.AMAT, 1)
        assert s.als.loss() < before
        s.free(); d.free(); sp.free()
        return True

    assert H.run_spmd(1, rank) == [True]


def test_everything_is_refused_on_the_plain_test_double():
    assert H.load_backend(T.ORACLE_BACKEND) == "oracle-cpu-test-double"
    case = small_case()

    def rank(world):
        s = IC.Solver(world, 1, case, False)
        s.set(case["A"], case["B"])
        named = r"Implicit_ALS.* needs the kernel hnh_(gemm_tn_f64|relu_grad_cols_f64|gram_rows_f64).*liboracle_backend\.so.*include/hnh_(grad|als_implicit)\.h"
        for folded in (False, True):
            s.als.set_folded(folded)
            for call in (lambda: s.als.half_step(H.AMAT, 1), lambda: s.als.run(1, 1), s.als.loss, lambda: s.als.gram(H.BMAT)):
                with pytest.raises(H.HnhError, match=named):
                    call()
        a, b = s.get()
        assert np.array_equal(a, T.fill_local(s.subA, a.shape, case["A"])) and np.array_equal(b, T.fill_local(s.subB, b.shape, case["B"]))
        s.free()
        return True

    assert H.run_spmd(1, rank) == [True]


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=als_common.case_id)
def test_composed_mode_meets_the_model_without_a_race(gat_double, case):
    g, R, p, c = case
    assert drain(gat_double) == (0, ""), "reports left behind by an earlier test"
    before = gat_double.hnh_oracle_order_accesses()
    IC.run_case(g, R, p, c, folded=False)
    assert drain(gat_double) == (0, ""), "no race and no MISUSE"
    assert gat_double.hnh_oracle_order_accesses() > before, "the case was watched"


def test_the_cases_are_the_ones_listed():
    assert len(OPERATOR_CASES) == len(set(OPERATOR_CASES)) == 13
    for g, R, p, c in OPERATOR_CASES:
        assert T.valid_config(IC.ALG, p, c, R)


def test_distributed_als_is_untouched_by_an_implicit_als_beside_it(gat_double):
    """A DistributedALS run before and after an ImplicitALS on the same operator returns the bits it returned alone: nothing stays lent."""
    R, p = 8, 4
    case, icase = als_common.inputs("hub", R, "forced"), IR.inputs("hub", R)

    def als_run(s):
        s.set(case["A"], case["B"])
        s.als.cg_optimizer(H.AMAT, 2); s.als.cg_optimizer(H.BMAT, 2)
        return s.get() + (s.als.computeResidual(),)

    def alone(world):
        s = als_common.Solver(world, IC.ALG, 1, case)
        out = als_run(s)
        s.free()
        return out

    def beside(world):
        s = als_common.Solver(world, IC.ALG, 1, case)
        first = als_run(s)
        ials = H.ImplicitALS(s.d, IR.LAMBDA)
        ws = IC.keyed(world, s.d, icase, s.subA, s.subB, icase["w"])
        ials.set_confidence(ws[0], ws[1]); ials.set_folded(False)
        s.set(icase["A"], icase["B"]); ials.set_embeddings(s.A, s.B)
        ials.run(1, 2)
        second = als_run(s)
        ials.free()
        for x in ws:
            x.free()
        s.free()
        return first, second

    want, got = H.run_spmd(p, alone), H.run_spmd(p, beside)
    for w, (first, second) in zip(want, got):
        for k in range(3):
            assert np.array_equal(w[k], first[k]) and np.array_equal(w[k], second[k])
