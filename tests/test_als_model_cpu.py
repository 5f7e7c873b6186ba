"""Holds tests/als_ref.py, the numpy definition of ALS-CG, down: it reproduces the reference's two golden runs, one of its iterations is
cg_common.reference_iteration, float64 is within a tenth of the operator tests' bound of long double on every input those tests use
(tests/als_common.py), and it tells three deliberately wrong solvers apart from the right one at that bound."""
import functools
import json
import os

import numpy as np
import pytest

import als_common as C
import als_ref
import cg_common
import hnh_testlib as T
from oracle import oracle as O

L = np.longdouble
CONDITION = T.ALS_TOL / 10     # the model's share of the bound, as test_gat_coef_cpu.py takes FTOL / 10 for its model


@pytest.mark.parametrize("name", ["er8_r16", "ragged_r8"])
def test_model_reproduces_the_reference_goldens(name):
    """1 alternating step of 5 CG iterations from the golden case's inputs: A, B and both residuals of the compiled reference."""
    case = T.case_inputs(name)
    gold = dict(np.load(os.path.join(T.GOLDEN, "als_%s.npz" % name)))
    a, b, res = als_ref.run(case["rows"], case["cols"], case["vals"], case["A"], case["B"], 1, 5)
    errs = dict(A=T.rel(a, gold["A"]), B=T.rel(b, gold["B"]), residuals=T.rel(res, gold["residuals"]))
    T.record_observed("als_model_vs_golden", case=name, **errs)
    print("als_ref vs golden %s: %s" % (name, errs))
    assert a.shape == gold["A"].shape and b.shape == gold["B"].shape and res.shape == gold["residuals"].shape
    assert max(errs.values()) <= T.ALS_TOL, errs


@pytest.mark.parametrize("hubs", [False, True])
@pytest.mark.parametrize("R", [7, 32])
def test_one_iteration_is_cg_common_reference_iteration(R, hubs):
    """On the operands cg_common.run builds for the kernel test (lambda = 1e-3, rsold not tied to r)."""
    rows, cols = (60, 6000) if hubs else (173, 400)
    rowptr, ridx, cidx = cg_common.block(rows, cols, R * 7 + hubs, hubs)
    rng = np.random.default_rng(R + 100)
    p, Y, x, r = (rng.uniform(-1, 1, (n, R)) for n in (rows, cols, rows, rows))
    rsold = np.einsum("ij,ij->i", r, r) * rng.uniform(0.5, 1.5, rows)
    lam, eps = 1e-3, 1e-8
    vals, Mp, wx, wr, wp, wrs = cg_common.reference_iteration(rowptr, ridx, cidx, p, Y, x, r, rsold, lam, eps)
    assert T.rel(als_ref.queries(ridx, cidx, p, Y, lam), Mp) <= 1e-13
    for got, want in zip(als_ref.cg_iteration(ridx, cidx, Y, x, r, p, rsold, lam, eps), (wx, wr, wp, wrs)):
        assert got.shape == want.shape and T.rel(got, want) <= 1e-13


def test_shapes_and_lengths_for_a_rectangular_matrix():
    """M != N: every matrix of the A half-step has M rows and every vector M entries, N for the B half-step; steps + 1 residuals."""
    m, n, R = 23, 41, 5
    rows, cols = O.erdos_renyi_mn(m, n, 150, 3)
    vals, A, B = O.sparse_values(rows, cols, n, 4), O.dense_fill(m, R, 5), O.dense_fill(n, R, 6)
    assert als_ref.rhs(rows, cols, vals, B, m).shape == (m, R) and als_ref.rhs(cols, rows, vals, A, n).shape == (n, R)
    assert als_ref.queries(rows, cols, A, B).shape == (m, R) and als_ref.queries(cols, rows, B, A).shape == (n, R)
    for (ri, ci, X, Y, nr) in ((rows, cols, A, B, m), (cols, rows, B, A, n)):
        new, trace = als_ref.half_step(ri, ci, vals, X, Y, 3, trace=True)
        assert new.shape == (nr, R) and len(trace) == 3
        for x, r, p, rsold in trace:
            assert x.shape == r.shape == p.shape == (nr, R) and rsold.shape == (nr,)
        assert np.array_equal(new, trace[-1][0])
    a, b, res = als_ref.run(rows, cols, vals, A, B, 2, 2)
    assert a.shape == (m, R) and b.shape == (n, R) and res.shape == (3,) and res[-1] < res[0]
    states = als_ref.forced(rows, cols, vals, A, B, 2, 2)
    assert [s[0] for s in states] == [0, 1, 0, 1] and [s[3].shape for s in states] == [(m, R), (n, R)] * 2
    fa, fb = states[-1][1], states[-1][3]   # free and forced running coincide in one precision
    assert np.array_equal(fa, a) and np.array_equal(fb, b)
    agt, bgt, a0, b0 = als_ref.hashed_init(m, n, R, 7)
    assert agt.shape == a0.shape == (m, R) and bgt.shape == b0.shape == (n, R)
    assert np.array_equal(a0, (O.hashed_uniform(np.arange(m * R, dtype=np.uint64), 10) * (1.4 / R)).reshape(m, R))
    assert np.max(np.abs(agt)) <= 1.0 / (R * m * R) and np.max(np.abs(b0)) <= 1.0 / (1.3 * R)


def test_the_graphs_are_what_the_cases_need():
    m, n, rows, cols = C.graph("hub")
    deg, degt = np.bincount(rows, minlength=m), np.bincount(cols, minlength=n)
    # rectangular; blocks with a remainder on grids of 8 (both sides) and of 6 (rows), exact quarters and fifths
    assert (m, n) == (1100, 2100) and m % 8 and n % 8 and m % 6 and 12000 < len(rows) < 12800
    assert np.all(rows[1:] * n + cols[1:] > rows[:-1] * n + cols[:-1])
    assert deg[1] >= 1500 and deg[m // 2] >= 1100 and degt[5] >= 1049 and np.sum(deg > C.LONG_ROW) == 2 and np.sum(degt > C.LONG_ROW) == 1 and deg[7] == 0 and degt[11] == 0
    # on 4 ranks every block of a hub row (of S and of S^T) is still longer than the segment path's threshold
    for hub_deg, other, size, nb in ((cols[rows == 1], n, n, 4), (cols[rows == m // 2], n, n, 4), (rows[cols == 5], m, m, 4)):
        per_block = np.bincount(hub_deg // -(-size // nb), minlength=nb)
        assert per_block.min() > C.LONG_ROW, per_block
    m, n, rows, cols = C.graph("rmat")
    deg, degt = np.bincount(rows, minlength=m), np.bincount(cols, minlength=n)
    assert 11500 < len(rows) < 12500 and (deg == 0).sum() > m // 6 and (degt == 0).sum() > n // 6 and deg.max() > C.LONG_ROW


# ------------------------------------------------------------------------------------------------ the condition
@functools.lru_cache(maxsize=None)
def long_double_answer(g, R, mode):
    c = C.inputs(g, R, mode)
    _, steps, iters = C.MODES[mode]
    fn = als_ref.run if mode == "free" else als_ref.forced
    return fn(c["rows"], c["cols"], c["vals"], c["A"], c["B"], steps, iters, L)


def condition(g, R, mode):
    """float64 model against the long-double model.  forced: both start every half-step from the long-double state rounded to
    float64, and again from the float64 model's own chain of states, which is what the operator tests upload."""
    c, want = C.inputs(g, R, mode), long_double_answer(g, R, mode)
    _, steps, iters = C.MODES[mode]
    if mode == "free":
        a, b, res = C.expected(g, R, mode)
        return max(T.rel(a, want[0]), T.rel(b, want[1]), T.rel(res, want[2]))
    worst = 0.0
    for (which, a_in, b_in, new), (_, a_own, b_own, new_own) in zip(want, C.expected(g, R, mode)):
        ridx, cidx = (c["cols"], c["rows"]) if which else (c["rows"], c["cols"])
        x, y = (b_in, a_in) if which else (a_in, b_in)
        worst = max(worst, T.rel(als_ref.half_step(ridx, cidx, c["vals"], x, y, iters), new))
        x, y = (b_own, a_own) if which else (a_own, b_own)
        worst = max(worst, T.rel(new_own, als_ref.half_step(ridx, cidx, c["vals"], x.astype(L), y.astype(L), iters)))
    return worst


@pytest.mark.parametrize("case", C.model_cases(), ids=C.case_id)
def test_float64_model_is_within_a_tenth_of_the_bound(case):
    g, R, mode = case
    err = condition(g, R, mode)
    T.record_observed("als_model_condition", graph=g, R=R, mode=mode, seeds=list(C.seeds(g, R, mode)), err=err)
    print("als_ref float64 vs long double %s R=%d %s: %.2e" % (g, R, mode, err))
    assert err <= CONDITION, (case, err)


def test_every_case_has_its_measured_condition_in_the_manifest():
    with open(os.path.join(T.GOLDEN, "als_manifest.json")) as f:
        mc = json.load(f)["model_condition"]
    for g, R, mode in C.model_cases():
        assert mc["measured"]["%s R%d %s" % (g, R, mode)] <= CONDITION
    assert mc["bound"] == CONDITION and all(len(s) == 3 for s in mc["seeds"].values())


# ------------------------------------------------------------------------------------------------ the model can tell
def iteration_without_the_constant_in_rsold(ridx, cidx, Y, x, r, p, rsold, lam, eps):
    """wrong on purpose: alpha sees rsold + eps, but the vector itself does not keep the constant (als .cpp:100 is in place)"""
    x, r, _, rsnew = als_ref.cg_iteration(ridx, cidx, Y, x, r, p, rsold, lam, eps)
    return x, r, r + (rsnew / rsold)[:, None] * p, rsnew


def iteration_that_loses_the_hub_row_epilogue(ridx, cidx, Y, x, r, p, rsold, lam, eps):
    """wrong on purpose: rows longer than 256 nonzeros miss p = r + beta p"""
    x, r, pnew, rsnew = als_ref.cg_iteration(ridx, cidx, Y, x, r, p, rsold, lam, eps)
    hub = np.bincount(ridx, minlength=len(x)) > C.LONG_ROW
    assert hub.any()
    pnew[hub] = p[hub]
    return x, r, pnew, rsnew


def wrong_answer(variant, g, R, mode):
    c = C.inputs(g, R, mode)
    _, steps, iters = C.MODES[mode]
    rows, cols, vals = c["rows"], c["cols"], c["vals"]
    if variant == "stale held operand":   # the A half-step of step 2 reads the B of step 1's start
        if mode == "forced":
            out = [list(s) for s in C.expected(g, R, mode)]
            out[2][3] = als_ref.half_step(rows, cols, vals, out[2][1], out[0][2], iters)
            return out
        A, B = c["A"], c["B"]
        res = [als_ref.residual(rows, cols, vals, A, B)]
        for step in range(steps):
            stale = B if step != 1 else prev_b
            prev_b = B
            A = als_ref.half_step(rows, cols, vals, A, stale, iters)
            B = als_ref.half_step(cols, rows, vals, B, A, iters)
            res.append(als_ref.residual(rows, cols, vals, A, B))
        return A, B, np.array(res)
    it = {"rsold loses the constant": iteration_without_the_constant_in_rsold,
          "lost hub-row epilogue": iteration_that_loses_the_hub_row_epilogue}[variant]
    half = functools.partial(als_ref.half_step, iteration=it)
    fn = als_ref.run if mode == "free" else als_ref.forced
    return fn(rows, cols, vals, c["A"], c["B"], steps, iters, np.float64, half=half)


def distance(g, R, mode, got):
    want = C.expected(g, R, mode)
    if mode == "free":
        return max(T.rel(got[0], want[0]), T.rel(got[1], want[1]), T.rel(got[2], want[2]))
    return max(T.rel(s[3], w[3]) for s, w in zip(got, want))


# the p update and the constant kept in rsold reach a factor only through a SECOND iteration: free mode (1 iteration) cannot see them
AFFECTS = {"stale held operand": ("free", "forced"), "rsold loses the constant": ("forced",), "lost hub-row epilogue": ("forced",)}
TELL_CASES = [("hub", 8), ("hub", 128), ("rmat", 128)]


@pytest.mark.parametrize("variant", list(AFFECTS))
def test_the_model_tells_a_wrong_solver_apart(variant):
    """Each wrong variant misses ALS_TOL by at least 10 x on at least one case of every mode it can affect; in a mode it cannot
    affect it is the model, bit for bit."""
    for mode in ("free", "forced"):
        d = {(g, R): distance(g, R, mode, wrong_answer(variant, g, R, mode)) for g, R in TELL_CASES}
        print("als_ref variant '%s' %s: %s" % (variant, mode, {k: "%.2e" % v for k, v in d.items()}))
        T.record_observed("als_model_variant", variant=variant, mode=mode, worst=max(d.values()), least=min(d.values()))
        if mode in AFFECTS[variant]:
            assert max(d.values()) >= 10 * T.ALS_TOL, (variant, mode, d)
        else:
            assert max(d.values()) == 0.0, (variant, mode, d)
