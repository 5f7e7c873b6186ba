"""The GAT's bias and skip connections on the GPU (include/hnh_gat_skip.h: HNH_ATTN_ADDEND on the finishing calls, hnh_skip_addend_cols_f64,
hnh_skip_grad_cols_f64, hnh_colsum_f64; GAT.set_bias / set_residual); tests/gat_skip_ref.py is the definition.

Kernel level, through ctypes: the finish of the four forward entry points (hnh_attn_softmax_csr_p, hnh_attn_add_fwd_csr_p,
hnh_attn_drop_fwd_csr_p, hnh_attn_v2_fwd_csr_p) with HNH_ATTN_ADDEND under relu, elu and the identity against the extended-precision
reference act_ld(o + addend) at the siblings' FTOL (1e-12 absolute), on their problem: 300 rows of 0 .. 16 nonzeros (some empty), gathered
values in [-50, 5], addends in [-2, 2], widths 1, 7, 64, 100, 128, 256 (and 384 for the dot-product softmax), aligned and at an odd offset.
Each on its own: empty rows give act(addend) (exactly for relu, the identity and the non-negative side of elu; within one unit of the
last place of the true expm1 below, where the device's expm1 and numpy's may round differently); a block with rowptr == NULL does the
same; lse and the row state are bit-equal to the call without the flag; a zero addend gives the bits of the call without the flag; the
six-window groupings are bit for bit (the destination is refilled before every run: the finish overwrites its addend); a mixed_degrees
block with hub rows; the flag without HNH_ATTN_FINISH returns HNH_ERR_INVALID and leaves guarded memory untouched.
The dense helpers: hnh_skip_grad_cols_f64 at rows {1, 5, 257} x f {1, 3, 7, 64, 100, 256} inside a three-head matrix with guard zones,
three activations, res null / a column block of a wider matrix / contiguous, bias null and set, against np.longdouble at the sibling's
1e-12 max|G|, dZ (both destinations) bit-equal to hnh_act_grad_cols_f64's, with saturated, zero, negative-zero and tiny outputs;
hnh_skip_addend_cols_f64 exact with its guards; hnh_colsum_f64 at rows {1, 257, 5000} x cols {1, 7, 256, 768} against np.longdouble at
rows eps max|src|, bit-identical on repeat.
Operator level: the three-layer model (12, 8, 2) projection, (16, 8, 2) identity, (16, 5, 3) projection with a bias on every layer and
activations elu, elu, identity on 15d_fusion2, c = 1 over 1, 2, 4, 8 loopback ranks on er8 and on the siblings' R-MAT graph with hub rows:
score additive with and without dropout, dot in both backward modes, gatv2; out, every dW, da, db, dW_res and dX against gat_skip_ref at
the siblings' TOL (1e-10); one layer at the benchmark head width 256 in each residual mode; everything off against gat_ref through the
existing harness and bit for bit against an object that never heard of the options; the refusals; attention_coefficients of a layer
unchanged by that layer's bias.  Training: the ten-step Adam trajectory against gat_skip_ref.train with the bounds of
test_gat_train_gpu.py (10 x the divergence of a reference run whose gradients are perturbed at 1e-10), the loss falls on
planted_partition, every parameter (bias and W_res included) bit-equal across ranks.

Every test prints its observed error before it asserts and records the worst case with T.record_observed.  Observed on an MI355X
(profiles/gat_skip_gputests.log): the finish with an addend at most 2.2e-14 (additive), 3.4e-14 (with dropout), 4.1e-14 (gatv2) and 3.6e-14
(dot-product softmax) absolute on the output and 4.6e-15 on lse, 1.0e-14 on the blocks with hub rows, against the 1e-12 bound; the dense
helper at most 2.7e-14 max|G| (delta; dZ 1.3e-16); the column sum at most 0.14 of rows eps max|src|; the operator at most 4.9e-15 (additive),
8.8e-14 (additive with dropout (0.6, 0.6)), 1.4e-15 (dot, both backward modes), 2.2e-14 (gatv2) on er8, 6.7e-15 on the R-MAT graph,
2.5e-15 at the head width 256 and 7.1e-15 with everything off, against 1e-10; the ten-step Adam trajectory at most 2.3e-15 in the
parameters (bound 2.5e-9) and 4.4e-16 in the loss (bound 2.2e-12); the training loss 1.442 -> 0.016 over LEARN_STEPS, held-out accuracy
0.959.  With W of scale 2 (the siblings' two-layer scale) the dropout case observed 1.1e-10 on this three-layer model: see
model_parameters for why that measures the inputs, and for the scale used instead."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_ref as R
import gat_skip_ref as S
import gat_v2_ref as V
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import (ALPHA, FTOL, FWD, GROUPINGS, NWIN, TOL, DropProblem, Problem, ctx, er8, hip_backend, same, setup, square_graph,  # noqa: F401
                             teardown)
from oracle import oracle as O
from test_gat_v2_gpu import V2Problem, padded

pytestmark = pytest.mark.gpu
BITS = {"relu": 0, "elu": K.ATTN_ACT_ELU, "identity": K.ATTN_ACT_IDENTITY}
ERR_INVALID = 1
M_ROWS, N_COLS = 300, 800
WIDTHS = [1, 7, 64, 100, 128, 256]
ULP_BELOW_ONE = 2.0 ** -53  # one unit of the last place of a value in (-1, -1/2], the largest in (-1, 0)


def short_degrees(seed, m=M_ROWS):
    """the siblings' rows: 0 .. 16 nonzeros, some rows empty, a fifth with one (their aggregate is the gathered row itself)"""
    d = np.random.default_rng(seed).integers(0, 17, m)
    d[::11] = 0
    d[1::5] = 1
    d[2] = 16
    return d


def abs_err(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)))


def act_of_addend_ok(got, addend, act):
    """act(addend) where a row has no nonzero: exact, but for elu below 0, where one unit of the last place of the true value is allowed"""
    if act == "relu":
        return np.array_equal(got, np.maximum(addend, 0.0))
    if act == "identity":
        return np.array_equal(got, addend + 0.0)
    pos = addend >= 0
    true = np.expm1(np.minimum(addend, 0.0).astype(np.longdouble))
    return np.array_equal(got[pos], addend[pos] + 0.0) and np.all(np.abs(got[~pos].astype(np.longdouble) - true[~pos]) <= ULP_BELOW_ONE)


# ------------------------------------------------------------------------------------------------ finish with addend: additive, dropout, gatv2
class AddendMixin:
    """The siblings' Problem classes with gathered values in [-50, 5], an addend in [-2, 2] waiting in the destination (out0, which run()
    writes back before every launch and checks the guards against) and the activation and addend bits ORed into every finishing call."""
    act, addend_bit = "relu", K.ATTN_ADDEND

    def prepare(self):
        f = self.f
        self.spread_gathered()
        self.out0 = np.random.default_rng(7000 + f).uniform(-2.0, 2.0, self.out0.shape)
        return self

    def spread_gathered(self):
        self.y[:, :self.f] = self.y[:, :self.f] * 27.5 - 22.5  # ([-1, 1] -> [-50, 5]; the scores' columns stay as they are)
        self.d["y"].set(self.y)

    def addend(self):
        return self.out0[:self.m, self.col0:self.col0 + self.f]

    def fn(self):
        real = super().fn()
        return lambda h, blk, a, flags, win, stream: real(h, blk, a, flags | ((BITS[self.act] | self.addend_bit) if flags & K.ATTN_FINISH else 0), win, stream)

    def raw_ld(self):
        return self.raw()


class AddAddend(AddendMixin, Problem):
    pass


class DropAddend(AddendMixin, DropProblem):
    pass


class V2Addend(AddendMixin, V2Problem):
    def spread_gathered(self):
        self.y = self.y * 27.5 - 22.5
        self.d["y"].set(padded(self.y, self.ld_y, self.off))

    def run(self, overwrite=True, groups=None):
        return super().run(overwrite, groups, act="relu")  # (the mixin's fn ORs the activation bits in)

    def raw_ld(self):
        return V.fwd_pass_ld(self.rows, self.colidx.astype(np.int64), self.m, self.x, self.y, self.a, self.f, ALPHA)


@contextlib.contextmanager
def degrees_for_v2(deg):
    """V2Problem draws its rows from gat_gpu_harness.mixed_degrees: hand it the given row lengths for one construction"""
    real = G.mixed_degrees
    G.mixed_degrees = lambda m, seed: deg
    try:
        yield
    finally:
        G.mixed_degrees = real


def make(ctx, kind, f, odd=False, seed=0, degrees=None):
    deg = short_degrees(f + seed) if degrees is None else degrees
    if kind == "v2":
        with degrees_for_v2(deg):
            return V2Addend(ctx, FWD, f, m=M_ROWS, ncols=N_COLS, seed=seed, odd=odd).prepare()
    cls = AddAddend if kind == "add" else DropAddend
    return cls(ctx, FWD, f, m=M_ROWS, ncols=N_COLS, seed=seed, odd=odd, degrees=deg).prepare()


KINDS = ["add", "drop", "v2"]


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_finish_with_addend_vs_extended_reference(ctx, kind, f, odd):
    p = make(ctx, kind, f, odd)
    o, lse = p.raw_ld()
    add = p.addend()
    deg = np.diff(p.rowptr)
    assert np.count_nonzero(deg == 0) > 20 and o.min() < -30 and o.max() > 1 and np.abs(add).max() > 1.5
    for act in ("relu", "elu", "identity"):
        p.act, p.addend_bit = act, K.ATTN_ADDEND
        got = p.run(True)  # (asserts the guards)
        want = R.act_ld(o + add.astype(np.longdouble), act)
        errs = (abs_err(got["out"], want), abs_err(got["lse"], lse))
        T.record_observed("gat_skip_kernel", case="%s f=%d%s %s" % (kind, f, " odd" if odd else "", act), worst=max(errs))
        print("observed", kind, f, odd, act, "out %.2e lse %.2e" % errs)
        assert max(errs) <= FTOL and not np.any(np.isnan(got["out"]))
        assert same(p.run(True), got), "a repeat must be bit-identical"
        assert act_of_addend_ok(got["out"][deg == 0], add[deg == 0], act), "a row without nonzeros: act(addend)"
        p.addend_bit = 0
        plain = p.run(True)
        assert np.array_equal(plain["lse"], got["lse"]) and np.array_equal(plain["state"], got["state"]), "lse and the row state do not see the flag"
        assert not np.array_equal(plain["out"], got["out"])
    p.free()


@pytest.mark.parametrize("f", [7, 64, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_zero_addend_is_the_call_without_the_flag(ctx, kind, f):
    p = make(ctx, kind, f, seed=1)
    p.out0[:p.m, p.col0:p.col0 + f] = 0.0
    for act in ("relu", "elu", "identity"):
        p.act, p.addend_bit = act, K.ATTN_ADDEND
        with_flag = p.run(True)
        p.addend_bit = 0
        assert same(p.run(True), with_flag), act
    p.free()


@pytest.mark.parametrize("f", [7, 128, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_grouping_independence_with_addend(ctx, kind, f):
    p = make(ctx, kind, f, seed=3)
    p.act = "elu"
    whole = p.run(True)
    for name, groups in GROUPINGS.items():
        assert same(p.run(True, groups), whole), name  # (run() refills the destination with the addend before every pass)
    p.free()


@pytest.mark.parametrize("kind", KINDS)
def test_hub_rows_with_addend(ctx, kind):
    f = 64
    deg = G.mixed_degrees(M_ROWS, 5)
    assert deg.max() >= 1500 and 600 in deg
    p = make(ctx, kind, f, degrees=deg)
    o, lse = p.raw_ld()
    p.act = "elu"
    got = p.run(True)
    errs = (abs_err(got["out"], R.act_ld(o + p.addend().astype(np.longdouble), "elu")), abs_err(got["lse"], lse))
    T.record_observed("gat_skip_kernel", case="%s f=%d hub rows elu" % (kind, f), worst=max(errs))
    print("observed hub rows", kind, "out %.2e lse %.2e" % errs)
    assert max(errs) <= FTOL
    for groups in GROUPINGS.values():
        assert same(p.run(True, groups), got)
    p.free()


def entry_point(p, kind):
    """the entry point without the mixin's bits"""
    return {"add": Problem.fn, "drop": DropProblem.fn, "v2": V2Problem.fn}[kind](p)


def reset(p):
    for k, v in (("out", p.out0), ("state", p.state0), ("acc", p.acc0)):
        p.d[k].set(v)


@pytest.mark.parametrize("kind", KINDS)
def test_null_rowptr_block_with_addend(ctx, kind):
    """rowptr == NULL resets and finishes every row to act(addend); after the nonzeros without a finish it finishes the rows to the whole
    pass's bits."""
    f = 33
    p = make(ctx, kind, f)
    a, call = p.args(), entry_point(p, kind)
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    add = p.addend()
    for act in ("relu", "elu", "identity"):
        p.act = act
        whole = p.run(True)
        bits = BITS[act] | K.ATTN_ADDEND
        reset(p)
        ctx.check(call(ctx.h, C.byref(none), C.byref(a), K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH | bits, None, K.STREAM_COMPUTE), "empty block, reset and finish")
        ctx.sync()
        out, state = p.d["out"].get(), p.d["state"].get()
        assert act_of_addend_ok(out[:p.m, p.col0:p.col0 + f], add, act) and np.all(state[2, :p.m] == 0.0)
        assert np.array_equal(out[:, :p.col0], p.out0[:, :p.col0]) and np.array_equal(out[:, p.col0 + f:], p.out0[:, p.col0 + f:]) and np.array_equal(out[p.m], p.out0[p.m])
        reset(p)
        ctx.check(call(ctx.h, C.byref(p.block()), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE), "the nonzeros")
        ctx.check(call(ctx.h, C.byref(none), C.byref(a), K.ATTN_FINISH | bits, None, K.STREAM_COMPUTE), "empty block, finish")
        ctx.sync()
        out, state = p.d["out"].get(), p.d["state"].get()
        assert np.array_equal(out[:p.m, p.col0:p.col0 + f], whole["out"]) and np.array_equal(state[2, :p.m], whole["lse"]), act
    p.free()


@pytest.mark.parametrize("kind", KINDS)
def test_addend_without_finish_is_refused_and_writes_nothing(ctx, kind):
    p = make(ctx, kind, 64)
    a, call = p.args(), entry_point(p, kind)
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    ov, add, elu = K.FUSED_OUT_OVERWRITE, K.ATTN_ADDEND, K.ATTN_ACT_ELU
    reset(p)
    for b in (p.block(), none):
        for flags in (add, ov | add, ov | add | elu):
            assert call(ctx.h, C.byref(b), C.byref(a), flags, None, K.STREAM_COMPUTE) == ERR_INVALID, flags
            assert b"HNH_ATTN" in ctx.lib.hnh_last_error(ctx.h)
    ctx.sync()
    assert np.array_equal(p.d["out"].get(), p.out0) and np.array_equal(p.d["state"].get(), p.state0) and np.array_equal(p.d["acc"].get(), p.acc0)
    p.free()


# ------------------------------------------------------------------------------------------------ finish with addend: the dot-product softmax
def softmax_problem(f, seed=0, degrees=None):
    m = M_ROWS
    rowptr, colidx, rows = square_graph(m, short_degrees(f + seed) if degrees is None else degrees, f + seed + 1)
    rng = np.random.default_rng(50 * f + seed)
    x = rng.uniform(-1, 1, (m, f)) * 0.2 / np.sqrt(f)  # scores of a few units
    y = rng.uniform(-1, 1, (m, f)) * 27.5 - 22.5       # gathered values in [-50, 5]
    dst0 = rng.uniform(-2.0, 2.0, (m + 1, f + 4 + (f & 1)))  # the addend in its head's block, guards round it
    return rowptr, colidx, rows, x, y, dst0


def softmax_pass(ctx, rowptr, colidx, x, y, dst0, off, bits, groups=None, null_block=False, zero_addend=False):
    """gat_gpu_harness.softmax_pass with a destination that holds dst0 before the pass (the addend in columns [off, off + R)), `bits` ORed
    into the finishing call, and the guard columns and the guard row checked against dst0.  null_block: the nonzeros in a call without
    a finish, then a block without nonzeros (rowptr == NULL) finishes.  Returns (output block, lse, row_max, row_sum, values)."""
    lib = ctx.lib
    m, R_ = x.shape
    nnz = int(rowptr[-1])
    ld = dst0.shape[1]
    if zero_addend:
        dst0 = dst0.copy()
        dst0[:m, off:off + R_] = 0.0
    drp, dci = ctx.upload(rowptr), ctx.upload(np.concatenate([colidx, [0]]).astype(np.int32))
    dx, dy = ctx.upload(x), ctx.upload(y)
    out = K.DevArray(ctx, m * R_, np.float64)
    vals = ctx.upload(np.full(max(nnz, 1), 3.0))
    rmax, rsum, lse = (ctx.upload(np.full(m, 5.0)) for _ in range(3))
    dst = ctx.upload(dst0)
    blk = K.CsrBlock(m, nnz, m, int(np.diff(rowptr).max()), 0, drp.ptr, dci.ptr, None)
    none = K.CsrBlock(m, 0, -1, 0, 0, None, None, None)
    st = K.AttnState(rmax.ptr, rsum.ptr, lse.ptr, ALPHA, dst.ptr + off * 8, ld)
    base = K.FUSED_VALUES_OVERWRITE

    def call(b, flags, win=None):
        ctx.check(lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(b), vals.ptr, dx.ptr, dy.ptr, out.ptr, R_, flags, C.byref(st), win, K.STREAM_COMPUTE), "softmax pass")

    if null_block:
        call(blk, base | K.FUSED_OUT_OVERWRITE)
        call(none, K.ATTN_FINISH | bits)
    elif groups is None:
        call(blk, base | K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH | bits)
    else:
        bounds = (C.c_int32 * (NWIN - 1))(*[int(m * (b + 1) / NWIN) for b in range(NWIN - 1)])
        split = K.DevArray(ctx, (NWIN - 1) * m, np.int32)
        ctx.check(lib.hnh_csr_window_bounds(ctx.h, m, drp.ptr, dci.ptr, NWIN - 1, bounds, split.ptr, K.STREAM_COMPUTE), "window bounds")
        for k, (a, b) in enumerate(groups):
            win = K.CsrWindow(None if a == 0 else split.ptr + (a - 1) * m * 4, None if b == NWIN else split.ptr + (b - 1) * m * 4, int(b == NWIN))
            call(blk, base | (K.FUSED_OUT_OVERWRITE if k == 0 else 0) | ((K.ATTN_FINISH | bits) if b == NWIN else 0), C.byref(win))
        ctx.sync()
        split.free()
    ctx.sync()
    d = dst.get()
    assert np.array_equal(d[:, :off], dst0[:, :off]) and np.array_equal(d[:, off + R_:], dst0[:, off + R_:]) and np.array_equal(d[m], dst0[m]), "guards"
    res = (d[:m, off:off + R_], lse.get(), rmax.get(), rsum.get(), vals.get()[:nnz])
    for a in (drp, dci, dx, dy, out, vals, rmax, rsum, lse, dst):
        a.free()
    return res


# (a width above 256 needs the 16-byte instances, hnh_attention.h: 384 has no odd-offset case)
SOFTMAX_CASES = [(f, off) for f in WIDTHS for off in (2, 3)] + [(384, 2)]


@pytest.mark.parametrize("f,off", SOFTMAX_CASES, ids=["f%d%s" % (f, "_odd-offset" if off % 2 else "") for f, off in SOFTMAX_CASES])
def test_softmax_finish_with_addend_vs_extended_reference(ctx, f, off):
    rowptr, colidx, rows, x, y, dst0 = softmax_problem(f)
    o, lse, _ = P.attention_ld(rows, colidx.astype(np.int64), M_ROWS, x, y, ALPHA)
    add = dst0[:M_ROWS, off:off + f]
    deg = np.diff(rowptr)
    assert o.min() < -30 and o.max() > 1 and np.count_nonzero(deg == 0) > 20
    for act in ("relu", "elu", "identity"):
        bits = BITS[act] | K.ATTN_ADDEND
        got = softmax_pass(ctx, rowptr, colidx, x, y, dst0, off, bits)
        errs = (abs_err(got[0], R.act_ld(o + add.astype(np.longdouble), act)), abs_err(got[1], lse))
        T.record_observed("gat_skip_kernel", case="softmax f=%d off=%d %s" % (f, off, act), worst=max(errs))
        print("observed softmax", f, off, act, "out %.2e lse %.2e" % errs)
        assert max(errs) <= FTOL and not np.any(np.isnan(got[0]))
        again = softmax_pass(ctx, rowptr, colidx, x, y, dst0, off, bits)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls must be bit-identical"
        assert act_of_addend_ok(got[0][deg == 0], add[deg == 0], act), "a row without nonzeros: act(addend)"
        plain = softmax_pass(ctx, rowptr, colidx, x, y, dst0, off, BITS[act])
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], plain[1:])), "lse, the row state and the scores do not see the flag"
        assert not np.array_equal(got[0], plain[0])
        zero = softmax_pass(ctx, rowptr, colidx, x, y, dst0, off, bits, zero_addend=True)
        assert all(np.array_equal(a, b) for a, b in zip(zero, plain)), "a zero addend: the bits of the call without the flag"
        nb = softmax_pass(ctx, rowptr, colidx, x, y, dst0, off, bits, null_block=True)
        assert all(np.array_equal(a, b) for a, b in zip(nb, got)), "a block with rowptr == NULL finishes the rows to the same bits"


@pytest.mark.parametrize("f", [7, 128, 256])
def test_softmax_grouping_independence_with_addend(ctx, f):
    rowptr, colidx, rows, x, y, dst0 = softmax_problem(f, seed=3)
    bits = K.ATTN_ACT_ELU | K.ATTN_ADDEND
    whole = softmax_pass(ctx, rowptr, colidx, x, y, dst0, 2, bits)
    for groups in GROUPINGS.values():
        if groups is not None:
            got = softmax_pass(ctx, rowptr, colidx, x, y, dst0, 2, bits, groups=groups)
            assert all(np.array_equal(a, b) for a, b in zip(got, whole)), groups


def test_softmax_hub_rows_with_addend(ctx):
    f = 64
    deg = G.mixed_degrees(M_ROWS, 5)
    rowptr, colidx, rows, x, y, dst0 = softmax_problem(f, degrees=deg)  # (a square block of 300 columns: a hub row repeats its pairs)
    o, lse, _ = P.attention_ld(rows, colidx.astype(np.int64), M_ROWS, x, y, ALPHA)
    assert np.diff(rowptr).max() >= 1500
    got = softmax_pass(ctx, rowptr, colidx, x, y, dst0, 2, K.ATTN_ACT_ELU | K.ATTN_ADDEND)
    errs = (abs_err(got[0], R.act_ld(o + dst0[:M_ROWS, 2:2 + f].astype(np.longdouble), "elu")), abs_err(got[1], lse))
    T.record_observed("gat_skip_kernel", case="softmax f=%d hub rows elu" % f, worst=max(errs))
    print("observed softmax hub rows out %.2e lse %.2e" % errs)
    assert max(errs) <= FTOL


def test_softmax_empty_block_and_flag_misuse(ctx):
    """rowptr == NULL with reset and finish: act(addend) everywhere; the addend bit without HNH_ATTN_FINISH leaves every destination as
    it was, on a block with nonzeros and on one without."""
    lib, f, off = ctx.lib, 33, 3
    m = M_ROWS
    rowptr, colidx, rows, x, y, dst0 = softmax_problem(f)
    ld, nnz = dst0.shape[1], int(rowptr[-1])
    none = K.CsrBlock(m, 0, -1, 0, 0, None, None, None)
    out0, vals0 = np.full(m * f, 2.0), np.full(nnz, 3.0)
    d = dict(rp=ctx.upload(rowptr), ci=ctx.upload(np.concatenate([colidx, [0]]).astype(np.int32)), x=ctx.upload(x), y=ctx.upload(y), out=ctx.upload(out0),
             vals=ctx.upload(vals0), rmax=ctx.upload(np.full(m, 5.0)), rsum=ctx.upload(np.full(m, 5.0)), lse=ctx.upload(np.full(m, 5.0)), dst=ctx.upload(dst0))
    blk = K.CsrBlock(m, nnz, m, int(np.diff(rowptr).max()), 0, d["rp"].ptr, d["ci"].ptr, None)
    st = K.AttnState(d["rmax"].ptr, d["rsum"].ptr, d["lse"].ptr, ALPHA, d["dst"].ptr + off * 8, ld)

    def call(b, flags):
        return lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(b), d["vals"].ptr, d["x"].ptr, d["y"].ptr, d["out"].ptr, f, flags, C.byref(st), None, K.STREAM_COMPUTE)

    vo, ov, add, elu = K.FUSED_VALUES_OVERWRITE, K.FUSED_OUT_OVERWRITE, K.ATTN_ADDEND, K.ATTN_ACT_ELU
    for b in (blk, none):
        for flags in (add, vo | ov | add, vo | ov | add | elu):
            assert call(b, flags) == ERR_INVALID, flags
            assert b"HNH_ATTN" in lib.hnh_last_error(ctx.h)
    ctx.sync()
    assert np.array_equal(d["dst"].get(), dst0) and np.array_equal(d["out"].get(), out0) and np.array_equal(d["vals"].get(), vals0)
    assert all(np.all(d[k].get() == 5.0) for k in ("rmax", "rsum", "lse"))
    for act in ("relu", "elu", "identity"):
        d["dst"].set(dst0)
        ctx.check(call(none, ov | K.ATTN_FINISH | BITS[act] | add), "empty block, reset and finish")
        ctx.sync()
        got = d["dst"].get()
        assert act_of_addend_ok(got[:m, off:off + f], dst0[:m, off:off + f], act) and np.all(d["lse"].get() == 0.0)
        assert np.array_equal(got[:, :off], dst0[:, :off]) and np.array_equal(got[:, off + f:], dst0[:, off + f:]) and np.array_equal(got[m], dst0[m])
    for v in d.values():
        v.free()


# ------------------------------------------------------------------------------------------------ hnh_skip_grad_cols_f64
def skip_grad_case(ctx, rows, f, act, even, res_kind, with_bias):
    """The sibling's act_grad_case with an addend: three heads of f columns in G, out and dZ_all (the middle one is the call's), dZ at its
    own pitch, delta with guards; res null, the middle column block of a three-head matrix, or a contiguous rows x f matrix; bias null or
    f entries inside a longer vector.  even = 1: every pitch and offset even (16-byte lanes when f is even); 0: odd pitches."""
    lib = ctx.lib
    rng = np.random.default_rng(1000 * rows + 10 * f + even)
    col0 = f + (f & 1) if even else f
    ld_g, ld_o, ld_dz, ld_all, ld_r = 3 * f + 4, 3 * f + 6, f + 2, 3 * f + 8, 3 * f + 2
    ld_g, ld_o, ld_dz, ld_all, ld_r = (v + (v % 2 if even else 1 - v % 2) for v in (ld_g, ld_o, ld_dz, ld_all, ld_r))
    g = rng.uniform(-3, 3, (rows, ld_g))
    res_full = rng.uniform(-1.5, 1.5, (rows + 1, ld_r))
    bias_full = rng.uniform(-0.5, 0.5, 3 * f + 2)
    b0 = col0  # (the bias of the middle head starts where its columns do: even when col0 is)
    res = None if res_kind == "none" else res_full[:rows, col0:col0 + f]
    bias = bias_full[b0:b0 + f] if with_bias else None
    addend = (0.0 if res is None else res) + (0.0 if bias is None else bias[None, :]) + np.zeros((rows, f))
    # the stored values' scale as in the sibling: the bound is absolute (1e-12 max|G|)
    o = rng.uniform(-40, 4, (rows, f)) if act != "identity" else (rng.uniform(-50, 5, (rows, f)) if f <= 7 else rng.uniform(-8, 4, (rows, f)))
    out = rng.uniform(-1, 1, (rows, ld_o))
    blk = R.act(o + addend, act)
    special = np.array([-1.0, 0.0, -0.0, -1.0 + 2.0 ** -53, -1e-300, 1e-300, -5e-324, -1e-17, 1e-17, -0.999999999999])
    flat = blk.reshape(-1)
    idx = rng.permutation(flat.size)[:min(flat.size, len(special))]
    flat[idx] = special[:len(idx)] if act != "relu" else np.abs(special[:len(idx)])
    out[:, col0:col0 + f] = flat.reshape(rows, f)
    dz0, all0, dl0 = np.full((rows + 1, ld_dz), 7.0), np.full((rows + 1, ld_all), 6.0), np.full(rows + 2, 9.0)
    d = dict(g=ctx.upload(g), out=ctx.upload(out), dz=ctx.upload(dz0), all=ctx.upload(all0), dl=ctx.upload(dl0), res=ctx.upload(res_full),
             resc=ctx.upload(np.ascontiguousarray(res_full[:rows, col0:col0 + f]) if rows * f else np.zeros(1)), bias=ctx.upload(bias_full))
    res_ptr, ld_res = {"none": (None, 0), "block": (d["res"].ptr + 8 * col0, ld_r), "contiguous": (d["resc"].ptr, f)}[res_kind]
    bias_ptr = d["bias"].ptr + 8 * b0 if with_bias else None

    def run(with_all=True):
        d["dz"].set(dz0)
        d["all"].set(all0)
        d["dl"].set(dl0)
        ctx.check(lib.hnh_skip_grad_cols_f64(ctx.h, d["dz"].ptr, ld_dz, d["all"].ptr if with_all else None, ld_all, d["dl"].ptr + 8, d["g"].ptr, ld_g,
                                             d["out"].ptr, ld_o, col0, res_ptr, ld_res, bias_ptr, rows, f, R.ACT_CODE[act], K.STREAM_COMPUTE),
                  "hnh_skip_grad_cols_f64")
        ctx.sync()
        return d["dz"].get(), d["all"].get(), d["dl"].get()

    dz, dza, dl = run()
    assert np.all(dz[:rows, f:] == 7.0) and np.all(dz[rows] == 7.0) and dl[0] == 9.0 and dl[rows + 1] == 9.0, "guards"
    assert np.all(dza[:, :col0] == 6.0) and np.all(dza[:, col0 + f:] == 6.0) and np.all(dza[rows] == 6.0), "guards of the second destination"
    assert np.array_equal(dza[:rows, col0:col0 + f], dz[:rows, :f]), "both destinations hold the same dZ"
    assert not np.any(np.isnan(dz[:rows, :f])) and not np.any(np.isnan(dl[1:rows + 1]))
    want_dz, want_dl = S.stored_grad(g[:, col0:col0 + f], out[:, col0:col0 + f], act, addend, np.longdouble)
    gmax = np.abs(g).max()
    errs = (abs_err(dz[:rows, :f], want_dz) / gmax, abs_err(dl[1:rows + 1], want_dl) / gmax)
    dz2, dza2, dl2 = run()
    assert np.array_equal(dz, dz2) and np.array_equal(dl, dl2) and np.array_equal(dza, dza2), "a second run must be bit-identical"
    dz3, dza3, dl3 = run(with_all=False)
    assert np.array_equal(dz, dz3) and np.array_equal(dl, dl3) and np.all(dza3 == 6.0), "the second destination is optional"
    d["dz"].set(dz0)
    d["dl"].set(dl0)
    ctx.check(lib.hnh_act_grad_cols_f64(ctx.h, d["dz"].ptr, ld_dz, d["dl"].ptr + 8, d["g"].ptr, ld_g, d["out"].ptr, ld_o, col0, rows, f, R.ACT_CODE[act],
                                        K.STREAM_COMPUTE), "hnh_act_grad_cols_f64")
    ctx.sync()
    assert np.array_equal(d["dz"].get(), dz), "dZ is hnh_act_grad_cols_f64's bit for bit"
    if res_kind == "none" and not with_bias:
        assert np.array_equal(d["dl"].get(), dl), "without an addend delta is hnh_act_grad_cols_f64's too"
    if act == "elu":
        assert np.all(dz[:rows, :f][out[:, col0:col0 + f] == -1.0] == 0.0)
    for v in d.values():
        v.free()
    return errs


@pytest.mark.parametrize("even", [1, 0], ids=["even-pitches", "odd-pitches"])
@pytest.mark.parametrize("f", [1, 3, 7, 64, 100, 256])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_skip_grad_cols_vs_extended_reference(ctx, rows, f, even):
    worst = {}
    for act in R.ACTIVATIONS:
        for res_kind in ("none", "block", "contiguous"):
            for with_bias in (False, True):
                worst[(act, res_kind, with_bias)] = skip_grad_case(ctx, rows, f, act, even, res_kind, with_bias)
    T.record_observed("gat_skip_grad", case="rows=%d f=%d even=%d" % (rows, f, even), worst=max(max(v) for v in worst.values()))
    print("observed skip_grad", rows, f, even, "dZ %.2e delta %.2e" % (max(v[0] for v in worst.values()), max(v[1] for v in worst.values())))
    # the sibling's bound: delta sums f terms of at most max|G| (max|o| + 2); f = 256 terms of 42 each stay far inside 1e-12 max|G|
    assert all(max(v) <= FTOL for v in worst.values()), worst


def test_skip_grad_cols_argument_checks(ctx):
    lib = ctx.lib
    buf = ctx.upload(np.full(256, 7.0))
    p = buf.ptr

    def call(dz=p, ld_dz=4, dza=p + 512, ld_all=8, dl=p + 1024, g=p, ld_g=8, out=p, ld_o=8, col0=2, res=p, ld_res=4, bias=p, rows=2, cols=4, act=1):
        return lib.hnh_skip_grad_cols_f64(ctx.h, dz, ld_dz, dza, ld_all, dl, g, ld_g, out, ld_o, col0, res, ld_res, bias, rows, cols, act, K.STREAM_COMPUTE)

    for kw in (dict(dz=None), dict(dl=None), dict(g=None), dict(out=None), dict(rows=-1), dict(cols=-1), dict(col0=-1), dict(col0=5), dict(ld_dz=3),
               dict(ld_g=5), dict(ld_o=5), dict(ld_all=5), dict(ld_res=3), dict(act=3), dict(act=-1), dict(dza=p)):
        assert call(**kw) == ERR_INVALID, kw
        assert b"hnh_skip_grad_cols_f64" in lib.hnh_last_error(ctx.h)
    assert call(rows=0) == 0
    ctx.sync()
    assert np.all(buf.get() == 7.0), "refused and empty calls write nothing"
    buf.free()


# ------------------------------------------------------------------------------------------------ hnh_skip_addend_cols_f64
@pytest.mark.parametrize("even", [1, 0], ids=["even-pitches", "odd-pitches"])
@pytest.mark.parametrize("f", [1, 7, 64, 100, 256])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_skip_addend_cols_is_exact(ctx, rows, f, even):
    lib = ctx.lib
    rng = np.random.default_rng(100 * rows + f + even)
    col0 = f + (f & 1) if even else f
    ld_d, ld_r = (v + (v % 2 if even else 1 - v % 2) for v in (3 * f + 4, f + 2))
    dst0 = rng.uniform(-1, 1, (rows + 1, ld_d))
    res = rng.uniform(-2, 2, (rows + 1, ld_r))
    bias = rng.uniform(-1, 1, f + 2)
    d = dict(dst=ctx.upload(dst0), res=ctx.upload(res), bias=ctx.upload(bias))
    for use_res in (False, True):
        for use_bias in (False, True):
            d["dst"].set(dst0)
            ctx.check(lib.hnh_skip_addend_cols_f64(ctx.h, d["dst"].ptr, ld_d, col0, d["res"].ptr if use_res else None, ld_r, d["bias"].ptr if use_bias else None,
                                                   rows, f, K.STREAM_COMPUTE), "hnh_skip_addend_cols_f64")
            ctx.sync()
            got = d["dst"].get()
            want = (res[:rows, :f] if use_res else 0.0) + (bias[None, :f] if use_bias else 0.0) + np.zeros((rows, f))
            assert np.array_equal(got[:rows, col0:col0 + f], want), (use_res, use_bias)
            assert np.array_equal(got[:, :col0], dst0[:, :col0]) and np.array_equal(got[:, col0 + f:], dst0[:, col0 + f:]) and np.array_equal(got[rows], dst0[rows])
    for kw in (dict(col0=-1), dict(col0=ld_d), dict(ld_r=f - 1), dict(rows=-1)):
        a = dict(col0=col0, ld_r=ld_r, rows=rows)
        a.update(kw)
        assert lib.hnh_skip_addend_cols_f64(ctx.h, d["dst"].ptr, ld_d, a["col0"], d["res"].ptr, a["ld_r"], None, a["rows"], f, K.STREAM_COMPUTE) == ERR_INVALID, kw
    for v in d.values():
        v.free()


# ------------------------------------------------------------------------------------------------ hnh_colsum_f64
@pytest.mark.parametrize("cols", [1, 7, 256, 768])
@pytest.mark.parametrize("rows", [1, 257, 5000])
def test_colsum_vs_extended_reference(ctx, rows, cols):
    lib = ctx.lib
    rng = np.random.default_rng(rows + cols)
    worst = 0.0
    for ld in (cols, cols + 3, cols + 4):
        src = rng.uniform(-3, 3, (rows, ld))
        need = lib.hnh_colsum_f64_workspace(rows, cols)
        assert 0 < need <= 512 * cols
        d = dict(src=ctx.upload(src), out=ctx.upload(np.full(cols + 2, 9.0)), work=ctx.upload(np.full(need + 1, 8.0)))

        def run():
            ctx.check(lib.hnh_colsum_f64(ctx.h, d["out"].ptr + 8, d["src"].ptr, ld, rows, cols, d["work"].ptr, need, K.STREAM_COMPUTE), "hnh_colsum_f64")
            ctx.sync()
            return d["out"].get()

        got = run()
        assert got[0] == 9.0 and got[cols + 1] == 9.0 and d["work"].get()[need] == 8.0, "guards"
        err = abs_err(got[1:cols + 1], src[:, :cols].astype(np.longdouble).sum(axis=0))
        bound = rows * np.finfo(np.float64).eps * np.abs(src).max()
        worst = max(worst, err / bound)
        assert err <= bound, (err, bound)
        assert np.array_equal(run(), got), "a repeat must be bit-identical"
        assert lib.hnh_colsum_f64(ctx.h, d["out"].ptr + 8, d["src"].ptr, ld, rows, cols, d["work"].ptr, need - 1, K.STREAM_COMPUTE) == ERR_INVALID
        assert lib.hnh_colsum_f64(ctx.h, d["out"].ptr + 8, d["src"].ptr, cols - 1, rows, cols, d["work"].ptr, need, K.STREAM_COMPUTE) == ERR_INVALID
        for v in d.values():
            v.free()
    T.record_observed("gat_skip_colsum", case="rows=%d cols=%d" % (rows, cols), worst=worst)
    print("observed colsum", rows, cols, "worst error / (rows eps max|src|) %.2e" % worst)


# ------------------------------------------------------------------------------------------------ the operator
LAYERS = [(12, 8, 2), (16, 8, 2), (16, 5, 3)]
RESIDUAL = ("projection", "identity", "projection")
ACTS = ("elu", "elu", "identity")


def model_parameters(layers, residual, score, seed=13, scale=1.0):
    """W of scale / sqrt(fan-in), vectors of order one, a bias in [-1, 1] on every layer and W_res of 1 / sqrt(fan-in) on every projection.
    The siblings' two-layer models use scale 2 to reach the negative side of ELU; here the bias and the residuals do that
    (assert_inputs_are_telling), and with three layers, an identity residual and dropout factors of 2.5 a scale of 2 grows the third
    layer's aggregates past 1500, where da1 = A^T ds is the difference of sums six orders larger: the numpy definition itself then moves
    by 1.2e-12 between true_grad and stored_grad (both fp64, gat_skip_ref.backward(from_stored=True)), 6.5e-15 at scale 1, and a
    comparison at 1e-10 would measure the inputs' conditioning."""
    rng = np.random.default_rng(seed)
    w = {(li, h): rng.standard_normal((fin, fph)) * scale / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    av = None
    if score == "additive":
        av = R.vectors_of(layers, seed=seed + 1)
    elif score == "gatv2":
        av = {k: (a, np.zeros_like(a)) for k, a in V.vectors_of(layers, seed=seed + 1).items()}
    bias = {li: rng.uniform(-1, 1, fph * heads) for li, (fin, fph, heads) in enumerate(layers)}
    wr = {li: rng.standard_normal((fin, fph * heads)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(layers) if residual[li] == "projection"}
    return w, av, bias, wr


def run_skip(world, rows, cols, m, x, layers, w, av, bias, wr, g, residual, score, rounds=1, **kw):
    """this rank's blocks and every round's results: gat_gpu_harness.one_round plus db and dW_res"""
    s = setup(world, rows, cols, m, x, layers, w, av, g, attention="softmax", score=score, residual=residual, bias=[li in bias for li in range(len(layers))], **kw)
    gnn = s["gnn"]
    for li, b in bias.items():
        gnn.set_bias(li, b)
    for li, r in wr.items():
        gnn.set_residual_weight(li, r)
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[])
    for _ in range(rounds):
        r = G.one_round(s, w, av is not None)
        r["db"] = {li: gnn.bias_grad(li) for li in bias}
        r["dwr"] = {li: gnn.residual_weight_grad(li) for li in wr}
        res["rounds"].append(r)
    teardown(s)
    return res


def assembled(per_rank, k, m, layers):
    got = G.assembled(per_rank, k, m, layers)
    r0 = per_rank[0]["rounds"][k]
    for pr in per_rank:
        assert all(np.array_equal(pr["rounds"][k]["db"][li], r0["db"][li]) for li in r0["db"]), "db must be equal on every rank"
        assert all(np.array_equal(pr["rounds"][k]["dwr"][li], r0["dwr"][li]) for li in r0["dwr"]), "dW_res must be equal on every rank"
    got.update(db=r0["db"], dwr=r0["dwr"])
    return got


def reference(rows, cols, m, x, layers, w, av, bias, wr, g, residual, score, acts=ACTS, rates=(0.0, 0.0), seed=0):
    mode = dict(score=score, rates=rates, seed=seed, activations=acts, residual=residual, bias=bias or None, res_weights=wr or None)
    dw, da, db, dwr, dx = S.backward(rows, cols, m, x, layers, ALPHA, g, w, av, **mode)
    return dict(out=S.forward(rows, cols, m, x, layers, ALPHA, w, av, **mode), dw=dw, da=da, db=db, dwr=dwr, dx=dx)


def compare(got, want, label, ranks, score):
    """out, every dW, da, db, dW_res and dX against the reference (max |x - ref| / max |ref| each, none vacuous); the worst is recorded
    and asserted <= TOL"""
    errs = {name: T.rel(got[name], want[name]) for name in ("out", "dx")}
    for key in want["dw"]:
        assert np.abs(want["dw"][key]).max() > 0
        errs[("dw",) + key] = T.rel(got["dw"][key], want["dw"][key])
    for key in want["da"]:
        pair = want["da"][key] if isinstance(want["da"][key], tuple) else (want["da"][key],)
        for i, v in enumerate(pair):
            assert np.abs(v).max() > 0
            errs[("da%d" % (i + 1),) + key] = T.rel(got["da"][key][i], v)
        if score == "gatv2":
            assert np.all(got["da"][key][1] == 0.0)
    for name in ("db", "dwr"):
        assert set(got[name]) == set(want[name])
        for li, v in want[name].items():
            assert np.abs(v).max() > 0
            errs[(name, li)] = T.rel(got[name][li], v)
    worst = max(errs.values())
    T.record_observed("gat_skip", case=label, ranks=ranks, worst=worst)
    print("observed gat_skip", label, ranks, "worst %.2e" % worst)
    assert worst <= TOL, errs


def assert_inputs_are_telling(rows, cols, m, x, layers, w, av, bias, wr, residual, score, acts):
    """the inputs' own check: a quarter of the hidden pre-activations negative, and |r + b| > |o| on a tenth of the units at least"""
    vec = {k: v[0] for k, v in av.items()} if score == "gatv2" else av
    pre = S.pre_activations(rows, cols, m, x, layers, ALPHA, w, vec, score=score, activations=acts, residual=residual, bias=bias, res_weights=wr)
    hidden = np.concatenate([(o + add).reshape(-1) for _, o, add in pre[:-1]]) if len(pre) > 1 else np.array([-1.0])
    o_all, add_all = (np.concatenate([p[i].reshape(-1) for p in pre]) for i in (1, 2))
    assert np.count_nonzero(hidden < 0) >= hidden.size // 4 and np.count_nonzero(np.abs(add_all) > np.abs(o_all)) >= o_all.size // 10


def er8_problem(score):
    rows, cols, m, _ = er8()
    x = O.dense_fill(m, LAYERS[0][0], 41) * 24.0  # (dense_fill is within 1/24: features of order one)
    w, av, bias, wr = model_parameters(LAYERS, RESIDUAL, score)
    if score == "dot":
        w = {k: v * 0.5 for k, v in w.items()}  # (dot-product scores are quadratic in W)
    g = O.dense_fill(m, LAYERS[-1][1] * LAYERS[-1][2], 9) * 16.0
    return rows, cols, m, x, w, av, bias, wr, g


CONFIGS = {"additive": dict(score="additive"), "additive dropout": dict(score="additive", dropout=(0.6, 0.6), seed=11),
           "dot unfused": dict(score="dot", backward="unfused"), "dot fused": dict(score="dot", backward="fused"), "gatv2": dict(score="gatv2")}
REFS, ER8 = {}, {}


def ref_vectors(av, score):
    return {k: v[0] for k, v in av.items()} if score == "gatv2" else av


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_operator_er8(p, config):
    kw = dict(CONFIGS[config])
    score = kw.pop("score")
    rows, cols, m, x, w, av, bias, wr, g = er8_problem(score)
    if config not in REFS:
        assert_inputs_are_telling(rows, cols, m, x, LAYERS, w, av, bias, wr, RESIDUAL, score, ACTS)
        REFS[config] = reference(rows, cols, m, x, LAYERS, w, ref_vectors(av, score), bias, wr, g, RESIDUAL, score, rates=kw.get("dropout", (0.0, 0.0)),
                                 seed=kw.get("seed", 0))
    per_rank = H.run_spmd(p, lambda wd: run_skip(wd, rows, cols, m, x, LAYERS, w, av, bias, wr, g, RESIDUAL, score, rounds=2, activation=ACTS, **kw))
    got = assembled(per_rank, 0, m, LAYERS)
    compare(got, REFS[config], "er8 %s p%d" % (config, p), p, score)
    again = assembled(per_rank, 1, m, LAYERS)
    assert np.array_equal(got["out"], again["out"]) and np.array_equal(got["dx"], again["dx"]), "two rounds must be bit-identical"
    assert all(np.array_equal(got["db"][li], again["db"][li]) for li in bias) and all(np.array_equal(got["dwr"][li], again["dwr"][li]) for li in wr)
    ER8[(p, config)] = got


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x, w, av, bias, wr, g = er8_problem("additive")
    res = {}
    for p in (1, 8):
        res[p] = ER8.get((p, "additive")) or assembled(H.run_spmd(p, lambda wd: run_skip(wd, rows, cols, m, x, LAYERS, w, av, bias, wr, g, RESIDUAL, "additive",
                                                                                          activation=ACTS)), 0, m, LAYERS)
    compare(res[8], res[1], "er8 additive p8 against p1", 8, "additive")


@pytest.mark.parametrize("score", ["additive", "dot", "gatv2"])
@pytest.mark.parametrize("p", [1, 4])
def test_operator_rmat_hub_rows(p, score):
    m = 1 << 13
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, LAYERS[0][0], 8) * 24.0
    w, av, bias, wr = model_parameters(LAYERS, RESIDUAL, score, seed=6)
    if score == "dot":
        w = {k: v * 0.5 for k, v in w.items()}
    g = O.dense_fill(m, LAYERS[-1][1] * LAYERS[-1][2], 4) * 32.0
    key = ("rmat", score)
    if key not in REFS:
        REFS[key] = reference(rows, cols, m, x, LAYERS, w, ref_vectors(av, score), bias, wr, g, RESIDUAL, score)
    kw = dict(backward="fused") if score == "dot" else {}
    per_rank = H.run_spmd(p, lambda wd: run_skip(wd, rows, cols, m, x, LAYERS, w, av, bias, wr, g, RESIDUAL, score, activation=ACTS, **kw))
    compare(assembled(per_rank, 0, m, LAYERS), REFS[key], "rmat hubs %s p%d" % (score, p), p, score)


@pytest.mark.parametrize("mode", ["none", "identity", "projection"])
def test_one_layer_at_the_benchmark_head_width(mode):
    """One layer of 256 inputs and one head of 256 features (the benchmark's head width), a bias, each residual mode, relu: the
    exact-width 16-byte instances of the finish and of the dense helpers."""
    m, layers = 1 << 11, [(256, 256, 1)]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, 256, 41) * 24.0
    w, av, bias, wr = model_parameters(layers, (mode,), "additive", seed=5, scale=6.0)
    g = O.dense_fill(m, 256, 3) * 64.0
    assert_inputs_are_telling(rows, cols, m, x, layers, w, av, bias, wr, (mode,), "additive", ("relu",))
    per_rank = H.run_spmd(1, lambda wd: run_skip(wd, rows, cols, m, x, layers, w, av, bias, wr, g, (mode,), "additive", activation=("relu",)))
    want = reference(rows, cols, m, x, layers, w, av, bias, wr, g, (mode,), "additive", acts=("relu",))
    compare(assembled(per_rank, 0, m, layers), want, "one layer f=256 residual %s" % mode, 1, "additive")


@pytest.mark.parametrize("p", [1, 4])
def test_everything_off_is_the_parent(p):
    """residual "none" and bias False spelled out, an object switched on and off again, and an object that never heard of the options:
    the same bits, output and gradients, and gat_ref's values through the existing harness."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w, av = G.hashed_weights(layers), R.vectors_of(layers)
    g = O.dense_fill(m, 12, 9) * 16.0
    mode = dict(attention="softmax", score="additive")

    def plain(world):
        return G.run_rounds(world, rows, cols, m, x, layers, w, av, g, **mode)

    def spelled(world):
        return G.run_rounds(world, rows, cols, m, x, layers, w, av, g, residual="none", bias=False, **mode)

    def trip(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, **mode)
        s["gnn"].forwardPass()
        s["gnn"].set_bias(0, np.ones(layers[0][1] * layers[0][2]))
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])  # a setter invalidates the stored forward pass
        s["gnn"].set_residual(1, "projection")
        mid = G.one_round(s, w, True)
        s["gnn"].set_bias(0, None)
        s["gnn"].set_residual(1, "none")
        after = G.one_round(s, w, True)
        teardown(s)
        return mid, after

    old, named, trips = H.run_spmd(p, plain), H.run_spmd(p, spelled), H.run_spmd(p, trip)
    for o, n, (mid, after) in zip(old, named, trips):
        o0 = o["rounds"][0]
        for a in (n["rounds"][0], after):
            assert np.array_equal(o0["out"], a["out"]) and np.array_equal(o0["dx"], a["dx"])
            assert all(np.array_equal(o0["dw"][k], a["dw"][k]) and np.array_equal(o0["da"][k][0], a["da"][k][0]) and
                       np.array_equal(o0["da"][k][1], a["da"][k][1]) for k in w)
        assert not np.array_equal(mid["out"], o0["out"]), "the round with a bias computed something else"
    G.compare(G.assembled(named, 0, m, layers), G.reference(rows, cols, m, x, layers, w, av, g, **mode), "gat_skip", "everything off p%d" % p, p)


@pytest.mark.parametrize("alg,attention,words", [("15d_fusion2", "none", "attention mode softmax only"), ("15d_fusion1", "softmax", "15d_fusion1.*c = 1")])
def test_refusals_leave_nothing_in_flight(alg, attention, words):
    rows, cols, m, x = er8()
    layers = [(16, 8, 2), (16, 4, 3)]

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, alg, sp, 16, 1)
        gnn = H.GAT(d, layers, ALPHA, attention=attention, residual=("identity", "none"), bias=(False, True))
        for k in [(li, h) for li, (_, _, heads) in enumerate(layers) for h in range(heads)]:
            gnn.set_weight(*k, O.gat_weight(k[0], k[1], layers[k[0]][0], layers[k[0]][1]))
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        for call in (gnn.forwardPass, lambda: gnn.backwardPass(g)):
            with pytest.raises(H.HnhError, match="residual identity of layer 0.*" + words):
                call()
        gnn.set_residual(0, "none")
        with pytest.raises(H.HnhError, match="bias of layer 1.*" + words):
            gnn.forwardPass()
        if alg == "15d_fusion2":  # (train_step and evaluate on 15d_fusion1 are refused for the loss's own reason first)
            gnn.set_labels(np.arange(m) % layers[-1][1], None, heads="mean")
            gnn.set_optimizer("adam", 0.01)
            for call in (gnn.train_step, gnn.evaluate):
                with pytest.raises(H.HnhError, match="bias of layer 1.*" + words):
                    call()
        world.sync()  # nothing was left in flight
        with pytest.raises(H.HnhError, match="input_features"):
            gnn.set_residual(1, "identity")
        with pytest.raises(ValueError):
            gnn.set_residual(0, "skip")
        gnn.set_bias(1, None)  # the object runs normally afterwards
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


@pytest.mark.parametrize("score", ["additive", "dot", "gatv2"])
def test_attention_coefficients_do_not_see_the_layers_own_bias(score):
    """The coefficients of a layer depend on its input and its W (and vectors) alone: a bias on that layer leaves them bit for bit, while
    the layer's output changes."""
    rows, cols, m, x, w, av, bias, wr, g = er8_problem(score)

    def rank(world):
        s = setup(world, rows, cols, m, x, LAYERS, w, av, g, attention="softmax", score=score, activation=ACTS)
        gnn = s["gnn"]
        gnn.forwardPass()
        gnn.get_output(s["out"])
        out0 = s["out"].download()
        last = len(LAYERS) - 1
        before = [gnn.attention_coefficients(last, h) for h in range(LAYERS[last][2])]
        vals0 = [v.download() for v in before]
        gnn.set_bias(last, bias[last])
        gnn.forwardPass()
        gnn.get_output(s["out"])
        out1 = s["out"].download()
        after = [gnn.attention_coefficients(last, h) for h in range(LAYERS[last][2])]
        vals1 = [v.download() for v in after]
        for v in before + after:
            v.free()
        teardown(s)
        return all(np.array_equal(a, b) for a, b in zip(vals0, vals1)) and not np.array_equal(out0, out1) and all(np.abs(v).max() > 0 for v in vals0)

    assert all(H.run_spmd(2, rank))


# ------------------------------------------------------------------------------------------------ training
ADAM = dict(kind="adam", lr=0.01, weight_decay=5e-4)
TRAIN_LAYERS = [(16, 8, 2), (16, 4, 3)]  # T.GAT_LAYERS' shapes with input_features == heads * features_per_head on layer 0
TRAIN_RESIDUAL = ("identity", "projection")
PUBLISHED = ("elu", "identity")


def train_problem(score):
    pp = R.planted_partition(TRAIN_LAYERS)
    rng = np.random.default_rng(21)
    bias = {li: rng.uniform(-0.5, 0.5, fph * heads) for li, (fin, fph, heads) in enumerate(TRAIN_LAYERS)}
    wr = {1: rng.standard_normal((16, 12)) / 4.0}
    av = pp["av"] if score == "additive" else {k: (v[0], np.zeros_like(v[0])) for k, v in pp["av"].items()}
    return pp, av, bias, wr


def device_train(world, pp, av, bias, wr, score, optimizer, steps):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], TRAIN_LAYERS, pp["w"], av, None, attention="softmax", score=score, activation=PUBLISHED,
              residual=TRAIN_RESIDUAL, bias=True)
    gnn = s["gnn"]
    for li, b in bias.items():
        gnn.set_bias(li, b)
    for li, r in wr.items():
        gnn.set_residual_weight(li, r)
    gnn.set_labels(pp["labels"], pp["mask"], heads="mean")
    opt = dict(optimizer)
    gnn.set_optimizer(opt.pop("kind"), opt.pop("lr"), **opt)
    res = dict(losses=[], accs=[])
    for _ in range(steps):
        loss, acc = gnn.train_step()
        res["losses"].append(loss)
        res["accs"].append(acc)
    res["w"] = {k: gnn.get_weight(*k) for k in pp["w"]}
    res["av"] = {k: gnn.get_attention_vectors(*k) for k in pp["w"]}
    res["bias"] = {li: gnn.get_bias(li) for li in bias}
    res["wr"] = {li: gnn.get_residual_weight(li) for li in wr}
    res["held"] = gnn.evaluate(~pp["mask"])
    teardown(s)
    return res


@pytest.mark.parametrize("score", ["additive", "gatv2"])
@pytest.mark.parametrize("p", [1, 4])
def test_adam_trajectory_with_bias_and_residuals(p, score):
    """Ten steps of train_step on gat_ref.planted_partition with an identity residual on the hidden layer, a projection on the output
    layer and a bias on both: within 10 x the divergence of a reference run whose gradients are perturbed at 1e-10 (the criterion of
    test_gat_train_gpu.py); the loss falls; every parameter, bias and W_res included, is bit-equal across the ranks and has moved."""
    pp, av, bias, wr = train_problem(score)
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], TRAIN_LAYERS, ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], ref_vectors(av, score))
    kw = dict(score=score, activations=PUBLISHED, residual=TRAIN_RESIDUAL, bias=bias, res_weights=wr)
    ref = S.train(*args, ADAM, 10, **kw)
    per = S.train(*args, ADAM, 10, perturb=(1e-10, np.random.default_rng(7)), **kw)
    bound_p = 10.0 * S.parameter_divergence(per, ref)
    bound_l = 10.0 * float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert bound_p > 0 and bound_l > 0
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, av, bias, wr, score, ADAM, 10))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        assert all(np.array_equal(pr["w"][k], r0["w"][k]) and np.array_equal(pr["av"][k][0], r0["av"][k][0]) and np.array_equal(pr["av"][k][1], r0["av"][k][1])
                   for k in r0["w"]), "parameters are bit-equal across ranks"
        assert all(np.array_equal(pr["bias"][li], r0["bias"][li]) for li in bias) and all(np.array_equal(pr["wr"][li], r0["wr"][li]) for li in wr)
    got_av = r0["av"] if score == "additive" else {k: v[0] for k, v in r0["av"].items()}
    got_p = S.parameter_divergence((None, None, r0["w"], got_av, r0["bias"], r0["wr"]), ref)
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_skip_trajectory", ranks=p, score=score, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l,
                      first=r0["losses"][0], last=r0["losses"][-1])
    print("observed gat_skip trajectory", score, p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l), r0["losses"])
    assert got_p <= bound_p and got_l <= bound_l and r0["accs"] == ref[1]
    assert r0["losses"][-1] < r0["losses"][0], "the planted-partition loss falls"
    assert all(np.abs(r0["bias"][li] - bias[li]).max() > 0 for li in bias) and all(np.abs(r0["wr"][li] - wr[li]).max() > 0 for li in wr), "bias and W_res are trained"


def test_learning_with_bias_and_residuals():
    pp, av, bias, wr = train_problem("additive")
    long_run = H.run_spmd(2, lambda wd: device_train(wd, pp, av, bias, wr, "additive", R.LEARN_OPTIMIZER, R.LEARN_STEPS))
    r0 = long_run[0]
    T.record_observed("gat_skip_learning", first=r0["losses"][0], last=r0["losses"][-1], held_out_accuracy=r0["held"][1])
    print("observed learning: loss %.3f -> %.3f, held-out accuracy %.3f" % (r0["losses"][0], r0["losses"][-1], r0["held"][1]))
    assert r0["losses"][-1] < r0["losses"][0]
    assert all(np.array_equal(pr["bias"][li], r0["bias"][li]) for pr in long_run for li in bias)
