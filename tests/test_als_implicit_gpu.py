"""Implicit-feedback ALS with confidence weights on the GPU (api.ImplicitALS; include/hnh_als_implicit.h: hnh_gram_rows_f64; tests/
als_implicit_ref.py is the definition).

The kernel alone against numpy at rows in {0, 1, 15, 16, 17, 63, 65, 1100} x R in {2, 8, 17, 100, 128, 130, 256} (no row, one row, either
side of a wave's 16-row tile, either side of two tiles, several workgroups with a remainder; every accumulator width with and without a
remainder in R, with and without 16-byte loads): without cg on small-integer operands Mp and rowdot are EXACT; with cg on the operands of a
real half-step x, r, p, rs come out within T.TOL, a row with rs == 0 and a row with bdot < 0 come back bit-identical (p = r), the guard
words around every buffer are intact, and two runs are bit-equal.
The operator in folded and composed mode against the definition at T.TOL (factors, Gram matrices, losses; every rank the same losses),
folded against composed at T.TOL; R = 257 runs composed and is refused folded; at R = 8, 32 iterations stay on the dense solve."""
import ctypes as C
import functools

import numpy as np
import pytest

import als_common
import als_implicit_common as IC
import als_implicit_ref as IR
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 15, 16, 17, 63, 65, 1100)
WIDTHS = (2, 8, 17, 100, 128, 130, 256)
KERNEL_CASES = [(rows, R) for rows in ROWS for R in WIDTHS]
OPERATOR_CASES = [("hub", R, p, 1) for R in (8, 17, 128, 256) for p in (1, 4)] + [("hub", 100, 5, 1), ("hub", 100, 4, 2), ("rmat", 128, 1, 1)]
GUARD = 16           # doubles in front of and behind every buffer (128 bytes: the buffers keep their alignment)
SENTINEL = -7.25e77


class Guarded:
    """A device buffer with guard words on both sides"""

    def __init__(self, ctx, arr):
        self.shape = arr.shape
        flat = np.concatenate([np.full(GUARD, SENTINEL), np.asarray(arr, dtype=np.float64).reshape(-1), np.full(GUARD, SENTINEL)])
        self.dev = ctx.upload(flat)
        self.ptr = self.dev.ptr + 8 * GUARD

    def get(self):
        flat = self.dev.get()
        assert np.all(flat[:GUARD] == SENTINEL) and np.all(flat[len(flat) - GUARD:] == SENTINEL), "guard words overwritten"
        return flat[GUARD:len(flat) - GUARD].reshape(self.shape)

    def free(self):
        self.dev.free()


def gram_rows(ctx, out, x, g, rows, R, rowdot=None, cg=None):
    lib = K.load()
    rc = lib.hnh_gram_rows_f64(ctx.h, out.ptr, x.ptr, g.ptr, rows, R, rowdot.ptr if rowdot else None, C.byref(cg) if cg else None, K.STREAM_COMPUTE)
    ctx.check(rc, "hnh_gram_rows_f64")


@functools.lru_cache(maxsize=None)
def half_step_state(R):
    """The operands of the first CG iteration of the A half-step of hub at width R, in numpy: (Out = sum w <p, y> y + lambda p, G, x, r, p, rs)"""
    c = IR.inputs("hub", R)
    rows, cols, w, x, y = c["rows"], c["cols"], c["w"], c["A"], c["B"]
    gram = y.T @ y
    rhs = IR.scatter_rows(rows, (1 + w)[:, None] * y[cols], x.shape[0])
    r = rhs - IR.apply_m(rows, cols, w, x, y, gram, IR.LAMBDA)
    p = r.copy()
    out = IR.apply_m(rows, cols, w, p, y, 0 * gram, IR.LAMBDA)
    return out, gram, x.copy(), r, p, IR.rowdot(r, r)


def cg_reference(out, gram, x, r, p, rs):
    mp = out + p @ gram
    bdot = IR.rowdot(p, mp)
    live = (rs > 0) & (bdot > 0)
    alpha = np.where(live, rs / np.where(live, bdot, 1), 0)
    xn = np.where(live[:, None], x + alpha[:, None] * p, x)
    rn = np.where(live[:, None], r - alpha[:, None] * mp, r)
    rsnew = IR.rowdot(rn, rn)
    beta = np.where(live, rsnew / np.where(live, rs, 1), 0)
    return xn, rn, np.where(live[:, None], rn + beta[:, None] * p, rn), rsnew, live


@pytest.mark.parametrize("rows,R", KERNEL_CASES, ids=lambda v: str(v))
def test_gram_rows_without_cg_is_exact_on_integers(ctx, rows, R):
    rng = np.random.default_rng(1000 * rows + R)
    x, g, out = (rng.integers(-4, 5, s).astype(np.float64) for s in ((rows, R), (R, R), (rows, R)))
    want = out + x @ g
    for with_dot in (True, False):
        bufs = [Guarded(ctx, a) for a in (out, x, g, np.full(max(rows, 1), SENTINEL))]
        gram_rows(ctx, bufs[0], bufs[1], bufs[2], rows, R, rowdot=bufs[3] if with_dot else None)
        got = [b.get() for b in bufs]
        assert np.array_equal(got[0], want) and np.array_equal(got[1], x) and np.array_equal(got[2], g)
        if with_dot:
            assert np.array_equal(got[3][:rows], IR.rowdot(x, want)) and np.all(got[3][rows:] == SENTINEL)
        else:
            assert np.all(got[3] == SENTINEL)
        for b in bufs:
            b.free()


@pytest.mark.parametrize("rows,R", KERNEL_CASES, ids=lambda v: str(v))
def test_gram_rows_with_cg_meets_numpy(ctx, rows, R):
    out, gram, x, r, p, rs = half_step_state(R)
    out, x, r, p, rs = (a[:rows].copy() for a in (out, x, r, p, rs))
    frozen, uphill = (1, 2) if rows >= 3 else (None, None)
    if rows >= 3:
        rs[frozen] = 0.0                                   # a row without residual
        out[uphill] = -(p[uphill] @ gram) - p[uphill]      # Mp = -p: bdot = -|p|^2 < 0
    xn, rn, pn, rsn, live = cg_reference(out, gram, x, r, p, rs)
    if rows >= 3:
        assert not live[frozen] and not live[uphill] and live.sum() == rows - 2
    results = []
    for _ in range(2):
        bufs = dict(out=Guarded(ctx, out), g=Guarded(ctx, gram), x=Guarded(ctx, x), r=Guarded(ctx, r), p=Guarded(ctx, p),
                    rs=Guarded(ctx, rs if rows else np.zeros(1)), dot=Guarded(ctx, np.full(max(rows, 1), SENTINEL)))
        cg = K.GramCg(bufs["x"].ptr, bufs["r"].ptr, bufs["p"].ptr, bufs["rs"].ptr)
        gram_rows(ctx, bufs["out"], bufs["p"], bufs["g"], rows, R, rowdot=bufs["dot"], cg=cg)
        got = {k: b.get() for k, b in bufs.items()}
        for b in bufs.values():
            b.free()
        results.append(got)
    got = results[0]
    for k in got:
        assert got[k].tobytes() == results[1][k].tobytes(), "two runs are bit-equal"
    assert np.array_equal(got["g"], gram) and np.all(got["dot"] == SENTINEL), "G is read only; rowdot is ignored with cg"
    if rows == 0:
        return
    errs = dict(x=T.rel(got["x"], xn), r=T.rel(got["r"], rn), p=T.rel(got["p"], pn), rs=T.rel(got["rs"], rsn))
    print("gram_rows cg rows=%d R=%d: %s" % (rows, R, " ".join("%s=%.2e" % kv for kv in errs.items())))
    assert max(errs.values()) <= T.TOL, errs
    for k in (frozen, uphill) if rows >= 3 else ():
        assert got["x"][k].tobytes() == x[k].tobytes() and got["r"][k].tobytes() == r[k].tobytes(), "a row that is not live keeps x and r"
        assert got["p"][k].tobytes() == r[k].tobytes(), "... and gets p = r"


def test_gram_rows_refusals(ctx):
    lib = K.load()
    a = ctx.upload(np.zeros((4, 257)))
    g = ctx.upload(np.zeros((257, 257)))
    for R, rows, cg, text in ((257, 4, None, b"wider than HNH_GRAM_MAX_R"), (0, 4, None, b"R < 1"), (8, -1, None, b"negative rows"),
                              (8, 4, K.GramCg(a.ptr, a.ptr, a.ptr, a.ptr), b"cg->p must be the call's X")):
        rc = lib.hnh_gram_rows_f64(ctx.h, a.ptr, g.ptr, g.ptr, rows, R, None, C.byref(cg) if cg else None, K.STREAM_COMPUTE)
        assert rc != 0 and text in lib.hnh_last_error(ctx.h), lib.hnh_last_error(ctx.h)
    a.free(); g.free()


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=als_common.case_id)
def test_both_modes_meet_the_model_and_each_other(case):
    g, R, p, c = case
    folded = IC.run_case(g, R, p, c, folded=True)
    composed = IC.run_case(g, R, p, c, folded=False)
    diff = max(T.rel(folded[k], composed[k]) for k in folded)
    print("als_implicit folded against composed: %.2e" % diff)
    assert diff <= T.TOL


def test_the_cases_are_the_ones_listed():
    assert len(KERNEL_CASES) == len(set(KERNEL_CASES)) == 56
    assert len(OPERATOR_CASES) == len(set(OPERATOR_CASES)) == 11
    for g, R, p, c in OPERATOR_CASES:
        assert T.valid_config(IC.ALG, p, c, R)


def test_wider_than_the_kernel_runs_composed_and_is_refused_folded():
    case = IR.inputs("hub", 257)
    want = IR.half_step(case["rows"], case["cols"], case["w"], case["A"], case["B"], IR.LAMBDA, 2)

    def rank(world):
        s = IC.Solver(world, 1, case, True)
        s.set(case["A"], case["B"])
        with pytest.raises(H.HnhError, match=r"folded mode supports R <= 256, not R = 257: use set_folded\(false\)"):
            s.als.half_step(H.AMAT, 2)
        s.als.set_folded(False)
        s.als.half_step(H.AMAT, 2)
        a, _ = s.get()
        s.free()
        return a

    got = H.run_spmd(1, rank)[0]
    assert T.rel(got[:case["M"]], want) <= T.TOL


@pytest.mark.parametrize("folded", [True, False], ids=["folded", "composed"])
def test_many_iterations_stay_on_the_dense_solve(folded):
    case = IR.inputs("hub", 8)
    want = IR.dense_solve(case["rows"], case["cols"], case["w"], case["B"], IR.LAMBDA, case["M"])

    def rank(world):
        s = IC.Solver(world, 1, case, folded)
        s.set(case["A"], case["B"])
        s.als.half_step(H.AMAT, 32)
        a, _ = s.get()
        s.free()
        return a

    got = H.run_spmd(1, rank)[0]
    err = T.rel(got[:case["M"]], want)
    print("als_implicit 32 iterations against the dense solve (%s): %.2e" % ("folded" if folded else "composed", err))
    assert np.all(np.isfinite(got)) and err <= T.TOL
