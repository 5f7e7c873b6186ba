"""The GAT's layer normalisation on the GPU (include/hnh_gat_norm.h: hnh_layernorm_fwd_f64, hnh_layernorm_bwd_f64,
hnh_layernorm_bwd_workspace; GAT.set_norm); tests/gat_norm_ref.py is the definition.

Kernel level, through ctypes, guard zones round every output.  Rows {1, 5, 257} x cols {1, 2, 7, 64, 100, 256, 768, 3584, 4096} (both
sides of the wave / workgroup switch at 512 columns with 16-byte accesses and 256 with 8-byte ones, every trip count, one and several
row ranges), pitches larger than cols, aligned and at an odd element offset (8-byte lanes), three activations, z in [-1, 1] and in
1000 + [-1, 1]:
    forward   against np.longdouble, per row |out - want| <= 32 eps64 (1 + max|z_r| / sigma_r) max(1, max|gamma|), sigma_r = sqrt(var_r + eps)
              (a float64 two-pass model stays within 0.73 of it, a one-pass E[z^2] - mu^2 variance misses it 70 - 1000 x on the shifted
              rows: test_gat_norm_cpu.py); mu within 4 eps64 max|z_r| and rstd within the same relative bound as out (its error is the
              deviations')
    backward  dz against np.longdouble, per row <= 128 eps64 (1 + max|z_r| / sigma_r) max|G| max|gamma| / sigma_r, from the device's
              own stats; dgamma and dbeta at rows {1, 257, 5000} x cols {1, 7, 256, 768} on the unshifted inputs (the shifted rows'
              conditioning belongs to xh, not to the sum) <= rows eps64 max|dY o xh| and rows eps64 max|dY|, the column-sum sibling's
              form.  The draws keep every |y| of the REFERENCE above 1e-9, so no gate can flip.
Exact cases: rows of the constant 3.0 give phi(beta) and stats (3, 1 / sqrt(eps)) (rstd: two correctly rounded operations, 2 eps64);
cols = 1 gives phi(beta); gamma = 1, beta = 0, identity gives xh; in-place calls bit-equal to out-of-place; repeats bit-identical;
rows = 0; cols = limit + 1 returns HNH_ERR_UNSUPPORTED with the guards intact; the workspace function agrees with what the backward
call accepts; overlaps other than the in-place ones are refused.

Operator level: the siblings' three-layer model (12, 8, 2) projection, (16, 8, 2) identity, (16, 5, 3) projection with a bias and a norm
(gamma in [0.5, 1.5], beta in [-1, 1]) on every layer, activations elu, elu, identity, 15d_fusion2, c = 1, 1, 2, 4, 8 loopback ranks, on er8
and on the siblings' R-MAT graph with hub rows and empty rows: score additive with and without dropout, dot in both backward modes, gatv2,
transformer with a learned edge bias; out, every existing gradient, dgamma, dbeta and dX against gat_norm_ref at the siblings' TOL
(1e-10); one layer of 14 heads of 256 (row width 3584); the norm on one layer only; the norm off everywhere bit-equal to an object that
never heard of it; attention_coefficients and evaluate on a normalised model; the refusals, with nothing left in flight.  Training: the
ten-step Adam trajectory against gat_norm_ref.train within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10
(the criterion of test_gat_train_gpu.py), with weight decay on and gamma / beta exempt in the reference; the loss falls on
planted_partition with the norm on the hidden layer; gamma and beta bit-equal across ranks; one SGD step with a large weight decay moves
gamma and beta by -lr times their gradients alone.

Every test prints its observed error before it asserts and records it with T.record_observed.  Observed on an MI355X
(profiles/gat_norm_gputests.log): the forward kernel at most 0.037 of its bound, dz 0.011 of its bound; the column sums at most 0.76 of
theirs, at rows = 1 (0.37 / 0.65 / 0.76 at 7 / 256 / 768 columns), 0.16 at 257 rows and 0.13 at 5000.  At rows = 1 there is no sum and the
bound is ONE eps64 of the largest term, less than the roundings of z - mu, its product with rstd and the product with dY taken together: a
plain float64 model misses it in a tenth of its draws (1.42 at worst over 300 draws at 1 x 256), and the kernel did (1.22 and 1.15 at
1 x 256 and 1 x 768) until it carried those products' low parts into the column sums.  The operator at most 5.8e-14 (er8, additive, 2 ranks)
against 1e-10; the ten-step Adam trajectory at most 7.3e-15 in the parameters (bound 4.3e-9) and 4.3e-16 in the loss (bound 8.8e-12); the
training loss 1.375 -> 0.024 over LEARN_STEPS, held-out accuracy 0.941; the undecayed SGD update of gamma and beta exact."""
import ctypes as C

import numpy as np
import pytest

import gat_gpu_harness as G
import gat_norm_ref as N
import gat_ref as R
import gat_v2_ref as V
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ALPHA, TOL, ctx, er8, hip_backend, setup, teardown  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
ERR_INVALID, ERR_UNSUPPORTED = 1, 4
ACTS3 = ("relu", "elu", "identity")
ROWS = [1, 5, 257]
COLS = [1, 2, 7, 64, 100, 256, 768, 3584, 4096]
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ kernel level
def draw(rows, cols, act, shift, seed):
    """z, gamma, beta, G whose reference has no |y| below 1e-9 (asserted on the reference), plus the reference in np.longdouble"""
    for k in range(50):
        rng = np.random.default_rng(100000 * seed + 1000 * k + 10 * rows + cols)
        z = shift + rng.uniform(-1, 1, (rows, cols))
        gamma, beta, g = rng.uniform(0.5, 1.5, cols), rng.uniform(-1, 1, cols), rng.uniform(-3, 3, (rows, cols))
        ref = N.ln_forward(z, gamma, beta, EPS, act, LD)
        if np.abs(ref[3]).min() >= 1e-9:
            return z, gamma, beta, g, ref
    raise AssertionError("no draw keeps the reference's y away from 0")


class NormCase:
    """One problem on the device: z, G, out and dz inside wider matrices of rows + 1 rows (pitches larger than cols; the pad columns and
    the last row are guards), stats, dgamma, dbeta and work with a guard double on either side.  odd=True moves every matrix base by one
    element and makes the pitches odd: 8-byte lanes."""

    def __init__(self, ctx, rows, cols, z, gamma, beta, g, odd, eps=EPS):
        self.ctx, self.rows, self.cols, self.odd, self.eps = ctx, rows, cols, odd, eps
        pad = (lambda v: v + 1 - v % 2) if odd else (lambda v: v + v % 2)
        self.ld_z, self.ld_o, self.ld_g, self.ld_dz = pad(cols + 4), pad(cols + 6), pad(cols + 2), pad(cols + 8)
        self.off = 1 if odd else 0
        rng = np.random.default_rng(7)
        self.host = {}
        for name, ld, src in (("z", self.ld_z, z), ("g", self.ld_g, g), ("out", self.ld_o, None), ("dz", self.ld_dz, None)):
            full = rng.uniform(5, 6, (rows + 1) * ld + 2)
            view = full[self.off:self.off + (rows + 1) * ld].reshape(rows + 1, ld)
            if src is not None:
                view[:rows, :cols] = src
            self.host[name] = full
        self.need = ctx.lib.hnh_layernorm_bwd_workspace(rows, cols)
        self.host.update(stats=np.full(2 * rows + 2, 9.0), gamma=np.concatenate([[7.0], gamma, [7.0]]), beta=np.concatenate([[7.0], beta, [7.0]]),
                         dgamma=np.full(cols + 2, 8.0), dbeta=np.full(cols + 2, 8.0), work=np.full(self.need + 2, 4.0))
        self.d = {k: ctx.upload(v) for k, v in self.host.items()}

    def ptr(self, name):
        return self.d[name].ptr + 8 * (self.off if name in ("z", "g", "out", "dz") else 1)

    def ld(self, name):
        return dict(z=self.ld_z, g=self.ld_g, out=self.ld_o, dz=self.ld_dz)[name]

    def matrix(self, name):
        """(the rows x cols block, True when every guard of the allocation still holds its fill)"""
        got = self.d[name].get()
        ld, rows, cols = self.ld(name), self.rows, self.cols
        keep = self.host[name]
        view = got[self.off:self.off + (rows + 1) * ld].reshape(rows + 1, ld)
        kview = keep[self.off:self.off + (rows + 1) * ld].reshape(rows + 1, ld)
        ok = (np.array_equal(view[:rows, cols:], kview[:rows, cols:]) and np.array_equal(view[rows], kview[rows]) and
              np.array_equal(got[:self.off], keep[:self.off]) and np.array_equal(got[self.off + (rows + 1) * ld:], keep[self.off + (rows + 1) * ld:]))
        return view[:rows, :cols].copy(), ok

    def vector(self, name, n, fill):
        got = self.d[name].get()
        return got[1:n + 1].copy(), bool(got[0] == fill and np.all(got[n + 1:] == fill))

    def forward(self, act, in_place=False, expect=0):
        lib, ctx = self.ctx.lib, self.ctx
        dst = "z" if in_place else "out"
        rc = lib.hnh_layernorm_fwd_f64(ctx.h, self.ptr(dst), self.ld(dst), self.ptr("z"), self.ld_z, self.ptr("stats"), self.ptr("gamma"), self.ptr("beta"),
                                       self.rows, self.cols, self.eps, R.ACT_CODE[act], K.STREAM_COMPUTE)
        assert rc == expect, (rc, lib.hnh_last_error(ctx.h))
        ctx.sync()
        out, ok = self.matrix(dst)
        stats, ok2 = self.vector("stats", 2 * self.rows, 9.0)
        assert ok and ok2, "guards of the forward call"
        return out, stats.reshape(self.rows, 2)

    def backward(self, act, in_place=False, expect=0, work_doubles=None):
        lib, ctx = self.ctx.lib, self.ctx
        dst = "g" if in_place else "dz"
        rc = lib.hnh_layernorm_bwd_f64(ctx.h, self.ptr(dst), self.ld(dst), self.ptr("dgamma"), self.ptr("dbeta"), self.ptr("g"), self.ld_g, self.ptr("z"),
                                       self.ld_z, self.ptr("stats"), self.ptr("gamma"), self.ptr("beta"), self.rows, self.cols, R.ACT_CODE[act],
                                       self.ptr("work"), self.need if work_doubles is None else work_doubles, K.STREAM_COMPUTE)
        assert rc == expect, (rc, lib.hnh_last_error(ctx.h))
        ctx.sync()
        dz, ok = self.matrix(dst)
        dgamma, ok2 = self.vector("dgamma", self.cols, 8.0)
        dbeta, ok3 = self.vector("dbeta", self.cols, 8.0)
        _, ok4 = self.vector("work", self.need, 4.0)
        assert ok and ok2 and ok3 and ok4, "guards of the backward call"
        return dz, dgamma, dbeta

    def reset(self, *names):
        for n in names:
            self.d[n].set(self.host[n])

    def free(self):
        for v in self.d.values():
            v.free()


def row_condition(z, rstd):
    return 1.0 + np.abs(z).max(axis=1) * rstd.astype(np.float64)


def check_case(ctx, rows, cols, act, shift, odd):
    """(forward error, dz error), each as a share of its bound"""
    z, gamma, beta, g, (want, (mu, rstd), xh, y) = draw(rows, cols, act, shift, 1)
    c = NormCase(ctx, rows, cols, z, gamma, beta, g, odd)
    out, stats = c.forward(act)
    cond = row_condition(z, rstd)
    f_bound = 32 * EPS64 * cond * max(1.0, np.abs(gamma).max())
    f_err = np.max(np.abs(out.astype(LD) - want), axis=1).astype(np.float64)
    mu_err = np.abs(stats[:, 0].astype(LD) - mu).astype(np.float64)
    rstd_err = np.abs(stats[:, 1].astype(LD) / rstd - 1).astype(np.float64)
    assert np.all(f_err <= f_bound), (np.max(f_err / f_bound), rows, cols, act, shift, odd)
    assert np.all(mu_err <= 4 * EPS64 * np.abs(z).max(axis=1)) and np.all(rstd_err <= 32 * EPS64 * cond)
    out2, stats2 = c.forward(act)
    assert np.array_equal(out, out2) and np.array_equal(stats, stats2), "a repeat must be bit-identical"
    # backward from the device's own stats
    want_dz, want_dg, want_db, dy = N.ln_backward(g, z, gamma, beta, EPS, act, LD)
    dz, dgamma, dbeta = c.backward(act)
    b_bound = 128 * EPS64 * cond * np.abs(g).max() * np.abs(gamma).max() * rstd.astype(np.float64)
    b_err = np.max(np.abs(dz.astype(LD) - want_dz), axis=1).astype(np.float64)
    assert np.all(b_err <= b_bound), (np.max(b_err / b_bound), rows, cols, act, shift, odd)
    dz2, dgamma2, dbeta2 = c.backward(act)
    assert np.array_equal(dz, dz2) and np.array_equal(dgamma, dgamma2) and np.array_equal(dbeta, dbeta2), "a repeat must be bit-identical"
    # in place: dz == G, then out == z (the operands are consumed, so these run last)
    dz3, dgamma3, dbeta3 = c.backward(act, in_place=True)
    assert np.array_equal(dz, dz3) and np.array_equal(dgamma, dgamma3) and np.array_equal(dbeta, dbeta3), "dz == G is bit-equal to out of place"
    c.reset("stats")
    out3, stats3 = c.forward(act, in_place=True)
    assert np.array_equal(out, out3) and np.array_equal(stats, stats3), "out == z is bit-equal to out of place"
    c.free()
    return float(np.max(f_err / f_bound)), float(np.max(b_err / b_bound))


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_vs_extended_reference(ctx, rows, cols):
    worst = [0.0, 0.0]
    for act in ACTS3:
        for shift in (0.0, 1000.0):
            for odd in ((False, True) if act == "elu" or rows == 5 else (False,)):  # (the 8-byte lanes: every shape, once per activation at least)
                f, b = check_case(ctx, rows, cols, act, shift, odd)
                worst = [max(worst[0], f), max(worst[1], b)]
    T.record_observed("gat_norm_kernels", case="rows=%d cols=%d" % (rows, cols), forward=worst[0], backward=worst[1])
    print("observed layernorm", rows, cols, "forward %.3f of its bound, dz %.3f of its bound" % tuple(worst))


@pytest.mark.parametrize("cols", [1, 7, 256, 768])
@pytest.mark.parametrize("rows", [1, 257, 5000])
def test_layernorm_column_sums_vs_extended_reference(ctx, rows, cols):
    worst = 0.0
    for act in ACTS3:
        for odd in (False, True):
            z, gamma, beta, g, (want, (mu, rstd), xh, y) = draw(rows, cols, act, 0.0, 2)
            c = NormCase(ctx, rows, cols, z, gamma, beta, g, odd)
            c.forward(act)
            _, want_dg, want_db, dy = N.ln_backward(g, z, gamma, beta, EPS, act, LD)
            _, dgamma, dbeta = c.backward(act)
            bg = rows * EPS64 * float(np.abs(dy * xh).max())
            bb = rows * EPS64 * float(np.abs(dy).max())
            eg = float(np.max(np.abs(dgamma.astype(LD) - want_dg)))
            eb = float(np.max(np.abs(dbeta.astype(LD) - want_db)))
            worst = max(worst, eg / bg if bg > 0 else 0.0, eb / bb if bb > 0 else 0.0)
            assert eg <= bg and eb <= bb, (eg, bg, eb, bb, act, odd)
            assert np.array_equal(c.backward(act)[1], dgamma), "a repeat must be bit-identical"
            c.free()
    T.record_observed("gat_norm_colsums", case="rows=%d cols=%d" % (rows, cols), worst=worst)
    print("observed layernorm column sums", rows, cols, "worst error / bound %.3f" % worst)


@pytest.mark.parametrize("cols", [1, 2, 100, 256, 768, 4096])
def test_layernorm_exact_cases(ctx, cols):
    rows = 5
    rng = np.random.default_rng(cols)
    gamma, beta = rng.uniform(0.5, 1.5, cols), rng.uniform(-1, 1, cols)
    for act in ACTS3:
        # rows of the constant 3.0: out = phi(beta) exactly (elu below 0: the device's expm1, one unit of the last place), stats (3, 1 / sqrt(eps))
        c = NormCase(ctx, rows, cols, np.full((rows, cols), 3.0), gamma, beta, np.ones((rows, cols)), False)
        out, stats = c.forward(act)
        want = N.ln_forward(np.zeros((1, cols)), np.ones(cols), beta, EPS, act, LD)[0][0]  # (phi(beta))
        exact = np.ones(cols, dtype=bool) if act != "elu" else beta >= 0
        assert np.array_equal(out[:, exact], np.broadcast_to(want.astype(np.float64)[exact], (rows, int(exact.sum()))))
        assert np.all(np.abs(out.astype(LD) - want[None, :]) <= 2.0 ** -53)
        assert np.all(stats[:, 0] == 3.0) and np.all(np.abs(stats[:, 1] * np.sqrt(EPS) - 1.0) <= 2 * EPS64)
        c.free()
    if cols == 1:  # one column: the deviation is 0 whatever z holds
        z = rng.uniform(-5, 5, (rows, 1))
        c = NormCase(ctx, rows, 1, z, gamma, beta, np.ones((rows, 1)), False)
        out, stats = c.forward("identity")
        assert np.all(out == beta[0]) and np.array_equal(stats[:, 0], z[:, 0])
        c.free()
    # gamma = 1, beta = 0, identity: xh itself
    z = rng.uniform(-1, 1, (rows, cols))
    c = NormCase(ctx, rows, cols, z, np.ones(cols), np.zeros(cols), np.ones((rows, cols)), False)
    out, stats = c.forward("identity")
    want, (mu, rstd), xh, _ = N.ln_forward(z, np.ones(cols), np.zeros(cols), EPS, "identity", LD)
    assert np.array_equal(out, (z - stats[:, :1]) * stats[:, 1:] + 0.0), "xh from the call's own stats, to the bit"
    assert np.all(np.max(np.abs(out.astype(LD) - xh), axis=1) <= 32 * EPS64 * row_condition(z, rstd))
    c.free()


def test_layernorm_edges_and_argument_checks(ctx):
    lib = ctx.lib
    rows, cols = 5, 8
    rng = np.random.default_rng(0)
    z, g = rng.uniform(-1, 1, (rows, cols)), rng.uniform(-1, 1, (rows, cols))
    c = NormCase(ctx, rows, cols, z, np.ones(cols), np.zeros(cols), g, False)
    out, stats = c.forward("relu")
    # the workspace function agrees with what the backward call accepts
    assert c.need == lib.hnh_layernorm_bwd_workspace(rows, cols) > 0
    c.backward("relu")
    c.reset("dz", "dgamma", "dbeta", "work")
    c.backward("relu", expect=ERR_INVALID, work_doubles=c.need - 1)  # (the guards are checked inside: nothing was written)
    for rows2, cols2 in ((1, 1), (257, 7), (5000, 768), (257, 3584), (1 << 18, 256)):
        assert lib.hnh_layernorm_bwd_workspace(rows2, cols2) % (2 * cols2) == 0 and lib.hnh_layernorm_bwd_workspace(rows2, cols2) > 0
    # rows = 0: the forward call writes nothing, the backward call zeros dgamma and dbeta alone
    p = c.ptr
    assert lib.hnh_layernorm_fwd_f64(ctx.h, p("out"), c.ld_o, p("z"), c.ld_z, p("stats"), p("gamma"), p("beta"), 0, cols, EPS, 0, K.STREAM_COMPUTE) == 0
    assert lib.hnh_layernorm_bwd_f64(ctx.h, p("dz"), c.ld_dz, p("dgamma"), p("dbeta"), p("g"), c.ld_g, p("z"), c.ld_z, p("stats"), p("gamma"), p("beta"), 0, cols, 0,
                                     None, 0, K.STREAM_COMPUTE) == 0
    ctx.sync()
    dgamma, ok = c.vector("dgamma", cols, 8.0)
    dbeta, ok2 = c.vector("dbeta", cols, 8.0)
    assert ok and ok2 and np.all(dgamma == 0.0) and np.all(dbeta == 0.0)
    assert np.array_equal(c.d["dz"].get(), c.host["dz"]) and np.array_equal(c.matrix("out")[0], out), "rows = 0 writes no matrix"
    # bad arguments and overlaps: refused, nothing written
    c.reset("out", "dz", "dgamma", "dbeta", "work", "stats")

    def fwd(out=p("out"), ld_o=c.ld_o, zz=p("z"), ld_z=c.ld_z, st=p("stats"), ga=p("gamma"), be=p("beta"), r=rows, cc=cols, eps=EPS, act=0):
        return lib.hnh_layernorm_fwd_f64(ctx.h, out, ld_o, zz, ld_z, st, ga, be, r, cc, eps, act, K.STREAM_COMPUTE)

    def bwd(dz=p("dz"), ld_dz=c.ld_dz, dg=p("dgamma"), db=p("dbeta"), gg=p("g"), ld_g=c.ld_g, zz=p("z"), ld_z=c.ld_z, st=p("stats"), ga=p("gamma"), be=p("beta"),
            r=rows, cc=cols, act=0, work=p("work"), n=c.need):
        return lib.hnh_layernorm_bwd_f64(ctx.h, dz, ld_dz, dg, db, gg, ld_g, zz, ld_z, st, ga, be, r, cc, act, work, n, K.STREAM_COMPUTE)

    for kw in (dict(out=None), dict(zz=None), dict(st=None), dict(ga=None), dict(be=None), dict(r=-1), dict(cc=-1), dict(ld_o=cols - 1), dict(ld_z=cols - 1),
               dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")), dict(act=3), dict(act=-1),
               dict(out=p("z") + 8), dict(out=p("z"), ld_o=c.ld_z + 2), dict(st=p("z")), dict(out=p("stats"))):
        assert fwd(**kw) == ERR_INVALID, kw
        assert b"hnh_layernorm_fwd_f64" in lib.hnh_last_error(ctx.h)
    for kw in (dict(dz=None), dict(dg=None), dict(db=None), dict(gg=None), dict(zz=None), dict(st=None), dict(ga=None), dict(be=None), dict(work=None),
               dict(r=-1), dict(cc=-1), dict(ld_dz=cols - 1), dict(ld_g=cols - 1), dict(ld_z=cols - 1), dict(act=3), dict(n=c.need - 1),
               dict(dz=p("g") + 8), dict(dz=p("z")), dict(dg=p("dbeta")), dict(work=p("dz")), dict(dg=p("gamma")), dict(dz=p("g"), ld_dz=c.ld_g + 2)):
        assert bwd(**kw) == ERR_INVALID, kw
        assert b"hnh_layernorm_bwd_f64" in lib.hnh_last_error(ctx.h)
    ctx.sync()
    for name in ("out", "dz", "dgamma", "dbeta", "work", "stats", "z", "g"):
        assert np.array_equal(c.d[name].get(), c.host[name]), "refused calls write nothing: " + name
    c.free()
    # one column past the limit: HNH_ERR_UNSUPPORTED, guards and everything else intact
    wide = K.NORM_MAX_COLS + 1
    c = NormCase(ctx, 2, wide, np.zeros((2, wide)), np.ones(wide), np.zeros(wide), np.ones((2, wide)), False)
    assert c.need == 0
    p = c.ptr
    assert lib.hnh_layernorm_fwd_f64(ctx.h, p("out"), c.ld_o, p("z"), c.ld_z, p("stats"), p("gamma"), p("beta"), 2, wide, EPS, 0, K.STREAM_COMPUTE) == ERR_UNSUPPORTED
    assert lib.hnh_layernorm_bwd_f64(ctx.h, p("dz"), c.ld_dz, p("dgamma"), p("dbeta"), p("g"), c.ld_g, p("z"), c.ld_z, p("stats"), p("gamma"), p("beta"), 2, wide, 0,
                                     p("work"), 2, K.STREAM_COMPUTE) == ERR_UNSUPPORTED
    ctx.sync()
    for name in ("out", "dz", "dgamma", "dbeta", "work", "stats"):
        assert np.array_equal(c.d[name].get(), c.host[name]), "an unsupported width writes nothing: " + name
    c.free()


# ------------------------------------------------------------------------------------------------ the operator
LAYERS = [(12, 8, 2), (16, 8, 2), (16, 5, 3)]
RESIDUAL = ("projection", "identity", "projection")
ACTS = ("elu", "elu", "identity")
CONFIGS = {"additive": dict(score="additive"), "additive dropout": dict(score="additive", dropout=(0.6, 0.6), seed=11),
           "dot unfused": dict(score="dot", backward="unfused"), "dot fused": dict(score="dot", backward="fused"), "gatv2": dict(score="gatv2"),
           "transformer learned edge bias": dict(score="transformer")}
REFS = {}


def edge_bias_fn(rows, cols):
    return 0.5 * np.sin(0.37 * np.asarray(rows, dtype=np.float64) + 0.11 * np.asarray(cols, dtype=np.float64))


def model_parameters(layers, residual, score, seed=13, edge=False, rows=None, cols=None, norms=None):
    """the siblings' parameters (W of 1 / sqrt(fan-in), vectors of order one, a bias in [-1, 1], W_res of 1 / sqrt(fan-in)) plus gamma in
    [0.5, 1.5] and beta in [-1, 1] on every normalised layer, as gat_norm_ref's one dictionary"""
    rng = np.random.default_rng(seed)
    heads = [(li, h, fin, fph) for li, (fin, fph, nh) in enumerate(layers) for h in range(nh)]
    p = {"w": {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, h, fin, fph in heads}}
    if score == "additive":
        p["av"] = R.vectors_of(layers, seed=seed + 1)
    elif score == "gatv2":
        p["av"] = V.vectors_of(layers, seed=seed + 1)
    elif score == "transformer":
        p["wq"] = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, h, fin, fph in heads}
        p["wk"] = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, h, fin, fph in heads}
        if edge:
            p["edge_bias"] = {li: edge_bias_fn(rows, cols) for li in range(len(layers))}
    elif score == "dot":
        p["w"] = {k: v * 0.5 for k, v in p["w"].items()}  # (dot-product scores are quadratic in W)
    p["bias"] = {li: rng.uniform(-1, 1, fph * nh) for li, (fin, fph, nh) in enumerate(layers)}
    p["wr"] = {li: rng.standard_normal((fin, fph * nh)) / np.sqrt(fin) for li, (fin, fph, nh) in enumerate(layers) if residual[li] == "projection"}
    on = [li for li in range(len(layers)) if norms is None or norms[li] == "layer"]
    p["gamma"] = {li: rng.uniform(0.5, 1.5, layers[li][1] * layers[li][2]) for li in on}
    p["beta"] = {li: rng.uniform(-1, 1, layers[li][1] * layers[li][2]) for li in on}
    return p


def configure(gnn, p, score):
    """every parameter of `p` beyond W and the vectors, which setup() has set"""
    for li, b in p.get("bias", {}).items():
        gnn.set_bias(li, b)
    for li, r in p.get("wr", {}).items():
        gnn.set_residual_weight(li, r)
    for li in p.get("gamma", {}):
        gnn.set_norm_weights(li, p["gamma"][li], p["beta"][li])
    for k in p.get("wq", {}):
        gnn.set_query_weight(*k, p["wq"][k])
        gnn.set_key_weight(*k, p["wk"][k])
    if "edge_bias" in p:
        gnn.edge_bias_from(edge_bias_fn)
        for li in p["edge_bias"]:
            gnn.set_edge_bias_learned(li, True)


def device_vectors(p, score):
    if score == "additive":
        return p["av"]
    return {k: (a, np.zeros_like(a)) for k, a in p["av"].items()} if score == "gatv2" else None


def run_norm(world, rows, cols, m, x, layers, p, g, score, norms, residual=RESIDUAL, acts=ACTS, rounds=1, **kw):
    """this rank's blocks and every round's results: gat_gpu_harness.one_round plus every other gradient"""
    s = setup(world, rows, cols, m, x, layers, p["w"], device_vectors(p, score), g, attention="softmax", score=score, residual=residual,
              bias=[li in p.get("bias", {}) for li in range(len(layers))], activation=acts, norm=norms, **kw)
    gnn = s["gnn"]
    configure(gnn, p, score)
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[])
    if "edge_bias" in p:
        res["coords"] = s["d"].S_coordinates()
    for _ in range(rounds):
        r = G.one_round(s, p["w"], "av" in p)
        r["bias"] = {li: gnn.bias_grad(li) for li in p.get("bias", {})}
        r["wr"] = {li: gnn.residual_weight_grad(li) for li in p.get("wr", {})}
        pairs = {li: gnn.norm_grad(li) for li in p.get("gamma", {})}
        r["gamma"], r["beta"] = {li: v[0] for li, v in pairs.items()}, {li: v[1] for li, v in pairs.items()}
        r["wq"] = {k: gnn.query_weight_grad(*k) for k in p.get("wq", {})}
        r["wk"] = {k: gnn.key_weight_grad(*k) for k in p.get("wq", {})}
        r["edge_bias"] = {li: gnn.edge_bias_grad(li)[0] for li in p.get("edge_bias", {})}
        res["rounds"].append(r)
    teardown(s)
    return res


REPLICATED = ("bias", "wr", "gamma", "beta", "wq", "wk")


def assembled(per_rank, k, m, layers, want_edge=None, pairs=None):
    got = G.assembled(per_rank, k, m, layers)
    r0 = per_rank[0]["rounds"][k]
    for pr in per_rank:
        for name in REPLICATED:
            assert all(np.array_equal(pr["rounds"][k][name][key], r0[name][key]) for key in r0[name]), name + " must be equal on every rank"
    got.update({name: r0[name] for name in REPLICATED})
    if want_edge is not None:  # every rank's share of dL/db against the reference's entry of the same (row, column): the worst per layer
        got["edge_err"] = {}
        for li, ref in want_edge.items():
            lookup = dict(zip(pairs.tolist(), ref.tolist()))
            worst = 0.0
            for pr in per_rank:
                rr, cc = pr["coords"]
                want = np.array([lookup[key] for key in (np.asarray(rr, dtype=np.int64) * m + np.asarray(cc, dtype=np.int64)).tolist()])
                if len(want):
                    worst = max(worst, float(np.max(np.abs(pr["rounds"][k]["edge_bias"][li] - want))))
            got["edge_err"][li] = worst / float(np.max(np.abs(ref)))
    return got


def reference(rows, cols, m, x, layers, p, g, score, norms, residual=RESIDUAL, acts=ACTS, rates=(0.0, 0.0), seed=0):
    mode = dict(score=score, rates=rates, seed=seed, activations=acts, residual=residual, norm=norms)
    want = N.backward(rows, cols, m, x, layers, ALPHA, g, p, **mode)
    want["out"] = N.forward(rows, cols, m, x, layers, ALPHA, p, **mode)
    return want


def compare(got, want, label, ranks, score):
    """out, every gradient and dX against the reference (max |x - ref| / max |ref| each, none vacuous); recorded, asserted <= TOL"""
    errs = {"out": T.rel(got["out"], want["out"]), "dx": T.rel(got["dx"], want["x"])}
    for key, v in want["w"].items():
        assert np.abs(v).max() > 0
        errs[("dw",) + key] = T.rel(got["dw"][key], v)
    for key, v in want.get("av", {}).items():
        for i, part in enumerate(v if isinstance(v, tuple) else (v,)):
            assert np.abs(part).max() > 0
            errs[("da%d" % (i + 1),) + key] = T.rel(got["da"][key][i], part)
        if score == "gatv2":
            assert np.all(got["da"][key][1] == 0.0)
    for name in REPLICATED:
        assert set(got[name]) == set(want.get(name, {})), name
        for key, v in want.get(name, {}).items():
            assert np.abs(v).max() > 0, (name, key)
            errs[(name, key)] = T.rel(got[name][key], v)
    for li, e in got.get("edge_err", {}).items():
        errs[("edge_bias", li)] = e
    worst = max(errs.values())
    T.record_observed("gat_norm", case=label, ranks=ranks, worst=worst)
    print("observed gat_norm", label, ranks, "worst %.2e" % worst)
    assert worst <= TOL, errs


def assert_inputs_are_telling(rows, cols, m, x, layers, p, mode):
    """the inputs' own check: the rows before the norm have a spread of order one and a mean that is not 0 (a norm that forgot mu, or that
    divided by 1, would be seen), and a quarter of the hidden norms' outputs sit on the negative side of the activation"""
    pre = N.pre_norm_rows(rows, cols, m, x, layers, ALPHA, p, **mode)
    for li, z in enumerate(pre):
        sd, mu = z.std(axis=1), np.abs(z.mean(axis=1))
        assert np.median(sd) > 0.05 and np.median(np.abs(sd - 1.0)) > 0.05 and np.median(mu) > 0.01, (li, np.median(sd), np.median(mu))
    _, trace = N.forward(rows, cols, m, x, layers, ALPHA, p, keep_trace=True, **mode)
    hidden = np.concatenate([t[2].reshape(-1) for t in trace[:-1]]) if len(trace) > 1 else np.array([-1.0])
    assert np.count_nonzero(hidden < 0) >= hidden.size // 4


def er8_problem(score, edge=False):
    rows, cols, m, _ = er8()
    x = O.dense_fill(m, LAYERS[0][0], 41) * 24.0  # (dense_fill is within 1/24: features of order one)
    p = model_parameters(LAYERS, RESIDUAL, score, edge=edge, rows=rows, cols=cols)
    g = O.dense_fill(m, LAYERS[-1][1] * LAYERS[-1][2], 9) * 16.0
    return rows, cols, m, x, p, g


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("ranks", [1, 2, 4, 8])
def test_operator_er8(ranks, config):
    kw = dict(CONFIGS[config])
    score = kw.pop("score")
    edge = "edge bias" in config
    rows, cols, m, x, p, g = er8_problem(score, edge)
    if config not in REFS:
        mode = dict(score=score, activations=ACTS, residual=RESIDUAL, norm="layer")
        assert_inputs_are_telling(rows, cols, m, x, LAYERS, p, mode)
        REFS[config] = reference(rows, cols, m, x, LAYERS, p, g, score, "layer", rates=kw.get("dropout", (0.0, 0.0)), seed=kw.get("seed", 0))
    per_rank = H.run_spmd(ranks, lambda wd: run_norm(wd, rows, cols, m, x, LAYERS, p, g, score, "layer", rounds=2, **kw))
    pairs = np.asarray(rows, dtype=np.int64) * m + np.asarray(cols, dtype=np.int64)
    if edge:
        assert len(np.unique(pairs)) == len(pairs), "the edge list names every pair once: a gradient per pair is well defined"
    got = assembled(per_rank, 0, m, LAYERS, REFS[config].get("edge_bias") if edge else None, pairs)
    compare(got, REFS[config], "er8 %s p%d" % (config, ranks), ranks, score)
    again = assembled(per_rank, 1, m, LAYERS)
    assert np.array_equal(got["out"], again["out"]) and np.array_equal(got["dx"], again["dx"]), "two rounds must be bit-identical"
    assert all(np.array_equal(got[n][li], again[n][li]) for n in ("gamma", "beta") for li in got[n])


@pytest.mark.parametrize("score", ["additive", "dot", "gatv2", "transformer"])
@pytest.mark.parametrize("ranks", [1, 4])
def test_operator_rmat_hub_rows(ranks, score):
    m = 1 << 13
    rows, cols = H.generate_rmat(13, m * 16)
    deg = np.bincount(rows, minlength=m)
    assert deg.max() >= 512 and np.bincount(cols, minlength=m).max() >= 512 and np.count_nonzero(deg == 0) > 0, "hub rows and empty rows"
    x = O.dense_fill(m, LAYERS[0][0], 8) * 24.0
    p = model_parameters(LAYERS, RESIDUAL, score, seed=6)
    g = O.dense_fill(m, LAYERS[-1][1] * LAYERS[-1][2], 4) * 32.0
    key = ("rmat", score)
    if key not in REFS:
        REFS[key] = reference(rows, cols, m, x, LAYERS, p, g, score, "layer")
    kw = dict(backward="fused") if score == "dot" else {}
    per_rank = H.run_spmd(ranks, lambda wd: run_norm(wd, rows, cols, m, x, LAYERS, p, g, score, "layer", **kw))
    compare(assembled(per_rank, 0, m, LAYERS), REFS[key], "rmat hubs %s p%d" % (score, ranks), ranks, score)


def test_one_layer_at_the_benchmark_row_width():
    """One layer of 14 heads of 256 features (the benchmark's 3584 values per row): the widest workgroup instances in the operator."""
    m, layers = 1 << 9, [(32, 256, 14)]
    rows, cols = H.generate_er(m, m, m * 8, 77)
    x = O.dense_fill(m, 32, 41) * 24.0
    p = model_parameters(layers, ("projection",), "additive", seed=5)
    g = O.dense_fill(m, 3584, 3) * 64.0
    args = dict(residual=("projection",), acts=("elu",))
    per_rank = H.run_spmd(1, lambda wd: run_norm(wd, rows, cols, m, x, layers, p, g, "additive", "layer", **args))
    want = reference(rows, cols, m, x, layers, p, g, "additive", "layer", **args)
    compare(assembled(per_rank, 0, m, layers), want, "one layer 14 x 256", 1, "additive")


def test_norm_on_one_layer_only():
    rows, cols, m, x, _, g = er8_problem("additive")
    norms = ("none", "layer", "none")
    p = model_parameters(LAYERS, RESIDUAL, "additive", norms=norms)
    per_rank = H.run_spmd(2, lambda wd: run_norm(wd, rows, cols, m, x, LAYERS, p, g, "additive", norms))
    want = reference(rows, cols, m, x, LAYERS, p, g, "additive", norms)
    assert set(want["gamma"]) == {1}
    compare(assembled(per_rank, 0, m, LAYERS), want, "er8 additive norm on layer 1 only", 2, "additive")


@pytest.mark.parametrize("ranks", [1, 4])
def test_norm_off_is_the_parent(ranks):
    """norm "none" spelled out, an object switched on and off again, and an object that never heard of the option: the same bits,
    output and gradients."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = G.hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, 12, 9) * 16.0
    mode = dict(attention="softmax", score="additive")

    def plain(world):
        return G.run_rounds(world, rows, cols, m, x, layers, w, av, g, **mode)

    def spelled(world):
        return G.run_rounds(world, rows, cols, m, x, layers, w, av, g, norm="none", **mode)

    def trip(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **mode)
        s["gnn"].forwardPass()
        s["gnn"].set_norm(0, "layer")
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])  # a setter invalidates the stored forward pass
        s["gnn"].set_norm_weights(0, np.full(layers[0][1] * layers[0][2], 1.5), np.full(layers[0][1] * layers[0][2], 0.25))
        mid = G.one_round(s, w, True)
        dgamma, dbeta = s["gnn"].norm_grad(0)
        s["gnn"].set_norm(0, "none")
        with pytest.raises(H.HnhError, match="no GAT norm gradient of layer 0"):
            s["gnn"].norm_grad(0)
        after = G.one_round(s, w, True)
        teardown(s)
        return mid, after, bool(np.abs(dgamma).max() > 0 and np.abs(dbeta).max() > 0)

    old, named, trips = H.run_spmd(ranks, plain), H.run_spmd(ranks, spelled), H.run_spmd(ranks, trip)
    for o, n, (mid, after, moved) in zip(old, named, trips):
        o0 = o["rounds"][0]
        for a in (n["rounds"][0], after):
            assert np.array_equal(o0["out"], a["out"]) and np.array_equal(o0["dx"], a["dx"])
            assert all(np.array_equal(o0["dw"][k], a["dw"][k]) and np.array_equal(o0["da"][k][0], a["da"][k][0]) and
                       np.array_equal(o0["da"][k][1], a["da"][k][1]) for k in w)
        assert moved and not np.array_equal(mid["out"], o0["out"]), "the round with the norm computed something else"
    G.compare(G.assembled(named, 0, m, layers), G.reference(rows, cols, m, x, layers, w, av, g, **mode), "gat_norm", "norm off p%d" % ranks, ranks)


@pytest.mark.parametrize("alg,attention,words", [("15d_fusion2", "none", "attention mode softmax only"), ("15d_fusion1", "softmax", "15d_fusion1.*c = 1")])
def test_refusals_leave_nothing_in_flight(alg, attention, words):
    rows, cols, m, x = er8()
    layers = [(16, 8, 2), (16, 4, 3)]

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, alg, sp, 16, 1)
        gnn = H.GAT(d, layers, ALPHA, attention=attention, norm=("layer", "none"))
        for k in [(li, h) for li, (_, _, heads) in enumerate(layers) for h in range(heads)]:
            gnn.set_weight(*k, O.gat_weight(k[0], k[1], layers[k[0]][0], layers[k[0]][1]))
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        for call in (gnn.forwardPass, lambda: gnn.backwardPass(g)):
            with pytest.raises(H.HnhError, match="norm layer of layer 0.*" + words):
                call()
        gnn.set_norm(0, "none")
        gnn.set_norm(1, "layer")
        with pytest.raises(H.HnhError, match="norm layer of layer 1.*" + words):
            gnn.forwardPass()
        if alg == "15d_fusion2":  # (train_step and evaluate on 15d_fusion1 are refused for the loss's own reason first)
            gnn.set_labels(np.arange(m) % layers[-1][1], None, heads="mean")
            gnn.set_optimizer("adam", 0.01)
            for call in (gnn.train_step, gnn.evaluate):
                with pytest.raises(H.HnhError, match="norm layer of layer 1.*" + words):
                    call()
        world.sync()  # nothing was left in flight
        with pytest.raises(ValueError):
            gnn.set_norm(0, "batch")
        with pytest.raises(ValueError):
            gnn.set_norm(0, "layer", eps=0.0)
        gnn.set_norm(1, "none")  # the object runs normally afterwards
        if attention == "softmax" and alg == "15d_fusion1":
            gnn.set_attention("none")
        d.setRValue(layers[0][0])
        x_d = H.Dense.create(world, *gnn.buffer_shape(0))
        x_d.upload(T.fill_local(d.submatrices(H.BMAT), x_d.shape, x))
        gnn.set_input(x_d)
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        gnn.get_output(out)
        ok = bool(np.isfinite(out.download()).all())
        for h in (out, x_d, g, gnn, d, sp):
            h.free()
        return ok

    assert all(H.run_spmd(2, rank))


def test_attention_coefficients_and_evaluate_on_a_normalised_model():
    """The coefficients of layer 1 are those of the reference's heads on layer 0's NORMALISED output (per pair of the edge list, which
    names every pair once), and evaluate gives the reference's loss and accuracy."""
    rows, cols, m, x, p, g = er8_problem("additive")
    labels = np.arange(m) % LAYERS[-1][1]
    mode = dict(score="additive", activations=ACTS, residual=RESIDUAL, norm="layer")
    out, trace = N.forward(rows, cols, m, x, LAYERS, ALPHA, p, keep_trace=True, **mode)
    want_loss, want_acc, _ = R.xent(out, labels, np.ones(m, dtype=bool), LAYERS[-1][2])
    pairs = np.asarray(rows, dtype=np.int64) * m + np.asarray(cols, dtype=np.int64)
    assert len(np.unique(pairs)) == len(pairs)
    want = [dict(zip(pairs.tolist(), trace[1][3][h][2].tolist())) for h in range(LAYERS[1][2])]

    def rank(world):
        s = setup(world, rows, cols, m, x, LAYERS, p["w"], p["av"], g, attention="softmax", score="additive", residual=RESIDUAL, bias=True, activation=ACTS,
                  norm="layer")
        gnn = s["gnn"]
        configure(gnn, p, "additive")
        gnn.set_labels(labels, None, heads="mean")
        loss, acc = gnn.evaluate()
        rr, cc = s["d"].S_coordinates()
        keys = (np.asarray(rr, dtype=np.int64) * m + np.asarray(cc, dtype=np.int64)).tolist()
        worst = 0.0
        for h in range(LAYERS[1][2]):
            v = gnn.attention_coefficients(1, h)
            vals = v.download()
            v.free()
            if len(keys):
                worst = max(worst, float(np.max(np.abs(vals - np.array([want[h][k] for k in keys])))))
        teardown(s)
        return loss, acc, worst

    res = H.run_spmd(2, rank)
    worst = max(max(abs(r[0] - want_loss) / abs(want_loss), r[2]) for r in res)
    T.record_observed("gat_norm_coefficients_evaluate", worst=worst)
    print("observed coefficients / evaluate on a normalised model: worst %.2e" % worst)
    assert worst <= TOL and all(r[1] == want_acc for r in res)


# ------------------------------------------------------------------------------------------------ training
ADAM = dict(kind="adam", lr=0.01, weight_decay=5e-4)
TRAIN_LAYERS = [(16, 8, 2), (16, 4, 3)]
TRAIN_RESIDUAL = ("identity", "projection")
PUBLISHED = ("elu", "identity")


def train_problem(score, norms):
    pp = R.planted_partition(TRAIN_LAYERS)
    rng = np.random.default_rng(21)
    p = {"w": pp["w"]}
    if score == "additive":
        p["av"] = pp["av"]
    else:
        p["wq"] = {k: rng.standard_normal(v.shape) / 4.0 for k, v in pp["w"].items()}
        p["wk"] = {k: rng.standard_normal(v.shape) / 4.0 for k, v in pp["w"].items()}
    p["bias"] = {li: rng.uniform(-0.5, 0.5, fph * heads) for li, (fin, fph, heads) in enumerate(TRAIN_LAYERS)}
    p["wr"] = {1: rng.standard_normal((16, 12)) / 4.0}
    on = [li for li in range(2) if norms[li] == "layer"]
    p["gamma"] = {li: rng.uniform(0.5, 1.5, TRAIN_LAYERS[li][1] * TRAIN_LAYERS[li][2]) for li in on}
    p["beta"] = {li: rng.uniform(-0.5, 0.5, TRAIN_LAYERS[li][1] * TRAIN_LAYERS[li][2]) for li in on}
    return pp, p


def read_parameters(gnn, p):
    got = {"w": {k: gnn.get_weight(*k) for k in p["w"]}}
    if "av" in p:
        got["av"] = {k: gnn.get_attention_vectors(*k) for k in p["av"]}
    if "wq" in p:
        got["wq"] = {k: gnn.get_query_weight(*k) for k in p["wq"]}
        got["wk"] = {k: gnn.get_key_weight(*k) for k in p["wk"]}
    got["bias"] = {li: gnn.get_bias(li) for li in p["bias"]}
    got["wr"] = {li: gnn.get_residual_weight(li) for li in p["wr"]}
    pairs = {li: gnn.get_norm_weights(li) for li in p["gamma"]}
    got["gamma"], got["beta"] = {li: v[0] for li, v in pairs.items()}, {li: v[1] for li, v in pairs.items()}
    return got


def device_train(world, pp, p, score, norms, optimizer, steps):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], TRAIN_LAYERS, p["w"], p.get("av"), None, attention="softmax", score=score, activation=PUBLISHED,
              residual=TRAIN_RESIDUAL, bias=True, norm=norms)
    gnn = s["gnn"]
    configure(gnn, p, score)
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    opt = dict(optimizer)
    gnn.set_optimizer(opt.pop("kind"), opt.pop("lr"), **opt)
    res = dict(losses=[], accs=[])
    for _ in range(steps):
        loss, acc = gnn.train_step()
        res["losses"].append(loss)
        res["accs"].append(acc)
    res["p"] = read_parameters(gnn, p)
    res["held"] = gnn.evaluate(~pp["mask"])
    teardown(s)
    return res


def same_parameters(a, b):
    fa, fb = N._flatten(a), N._flatten(b)
    return fa.keys() == fb.keys() and all(np.array_equal(fa[k], fb[k]) for k in fa)


@pytest.mark.parametrize("score", ["additive", "transformer"])
@pytest.mark.parametrize("ranks", [1, 4])
def test_adam_trajectory_with_the_norm(ranks, score):
    """Ten steps of train_step on gat_ref.planted_partition with the norm, a bias and a residual on both layers, weight decay on: within
    10 x the divergence of a reference run whose gradients are perturbed at 1e-10 (the criterion of test_gat_train_gpu.py).  The
    reference exempts gamma and beta from the decay: a product that decayed them would move them by lr-sized steps off the trajectory."""
    norms = ("layer", "layer")
    pp, p = train_problem(score, norms)
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], TRAIN_LAYERS, ALPHA, pp["labels"], pp["mask"], "mean", p)
    kw = dict(score=score, activations=PUBLISHED, residual=TRAIN_RESIDUAL, norm=norms)
    ref = N.train(*args, ADAM, 10, **kw)
    per = N.train(*args, ADAM, 10, perturb=(1e-10, np.random.default_rng(7)), **kw)
    bound_p = 10.0 * N.parameter_divergence(per[2], ref[2])
    bound_l = 10.0 * float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert bound_p > 0 and bound_l > 0
    per_rank = H.run_spmd(ranks, lambda wd: device_train(wd, pp, p, score, norms, ADAM, 10))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        assert same_parameters(pr["p"], r0["p"]), "every parameter, gamma and beta included, is bit-equal across ranks"
    got_p = N.parameter_divergence(r0["p"], ref[2])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_norm_trajectory", ranks=ranks, score=score, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l,
                      first=r0["losses"][0], last=r0["losses"][-1])
    print("observed gat_norm trajectory", score, ranks, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l), r0["losses"])
    assert got_p <= bound_p and got_l <= bound_l and r0["accs"] == ref[1]
    assert r0["losses"][-1] < r0["losses"][0], "the planted-partition loss falls"
    assert all(np.abs(r0["p"][n][li] - p[n][li]).max() > 0 for n in ("gamma", "beta") for li in p[n]), "gamma and beta are trained"


def test_learning_with_the_norm_on_the_hidden_layer():
    norms = ("layer", "none")
    pp, p = train_problem("additive", norms)
    long_run = H.run_spmd(2, lambda wd: device_train(wd, pp, p, "additive", norms, R.LEARN_OPTIMIZER, R.LEARN_STEPS))
    r0 = long_run[0]
    T.record_observed("gat_norm_learning", first=r0["losses"][0], last=r0["losses"][-1], held_out_accuracy=r0["held"][1])
    print("observed learning with the norm: loss %.3f -> %.3f, held-out accuracy %.3f" % (r0["losses"][0], r0["losses"][-1], r0["held"][1]))
    assert r0["losses"][-1] < r0["losses"][0]
    assert all(same_parameters(pr["p"], r0["p"]) for pr in long_run), "gamma and beta bit-equal across ranks after the steps"


def test_weight_decay_leaves_gamma_and_beta_alone():
    """One SGD step (no momentum) with weight decay 0.5: p' = p - lr (g + 0.5 p) for a decayed tensor, p' = p - lr g for gamma and beta.
    With lr = 0.1 a decayed gamma of order one would be off by 0.05; the undecayed update is reproduced to two roundings."""
    norms = ("layer", "layer")
    pp, p = train_problem("additive", norms)
    lr, wd = 0.1, 0.5

    def rank(world):
        s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], TRAIN_LAYERS, p["w"], p["av"], None, attention="softmax", score="additive", activation=PUBLISHED,
                  residual=TRAIN_RESIDUAL, bias=True, norm=norms)
        gnn = s["gnn"]
        configure(gnn, p, "additive")
        gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
        gnn.set_optimizer("sgd", lr, weight_decay=wd)
        gnn.forwardPass()
        gnn.loss(grad_out=s["g"])
        gnn.backwardPass(s["g"])
        grads = {li: gnn.norm_grad(li) for li in (0, 1)}
        db = {li: gnn.bias_grad(li) for li in (0, 1)}
        gnn.optimizer_step()
        after = {li: gnn.get_norm_weights(li) for li in (0, 1)}
        bias = {li: gnn.get_bias(li) for li in (0, 1)}
        teardown(s)
        return grads, after, db, bias

    for grads, after, db, bias in H.run_spmd(2, rank):
        for li in (0, 1):
            for q, name in enumerate(("gamma", "beta")):
                want = p[name][li] - lr * grads[li][q]
                err = float(np.max(np.abs(after[li][q] - want)))
                print("observed undecayed update of", name, li, "%.2e" % err)
                assert np.abs(grads[li][q]).max() > 0 and err <= 4 * EPS64 * max(1.0, np.abs(p[name][li]).max())
            assert np.max(np.abs(bias[li] - (p["bias"][li] - lr * (db[li] + wd * p["bias"][li])))) <= 4 * EPS64, "the bias is decayed, as before"
