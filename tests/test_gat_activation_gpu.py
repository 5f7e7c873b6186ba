"""The GAT's per-layer output activation on the GPU (the HNH_ATTN_ACT_* flags of include/hnh_attention.h, hnh_act_grad_cols_f64 of
include/hnh_grad.h, GAT.set_activation); tests/gat_ref.py with `activations` is the definition.

Kernel level, through ctypes: the finish of the three forward entry points (hnh_attn_softmax_csr_p, hnh_attn_add_fwd_csr_p,
hnh_attn_drop_fwd_csr_p) with ELU and the identity against the extended-precision references at 1e-12 ABSOLUTE (the forward tolerance of
the additive kernel tests; the activation amplifies nothing: |elu'| <= 1), on 300 rows of at most 16 nonzeros with gathered values in
[-50, 5], widths 1, 7, 64, 100, 128, 256 (and 384 for the dot-product softmax), aligned and at an odd offset; the six-window groupings bit
for bit; blocks without nonzeros; the refused flag combinations; the ReLU default against the same call's identity output.  The dense
backward helper at rows {1, 5, 257} x f {1, 3, 7, 64, 100, 256} inside a three-head matrix with guards, against np.longdouble at
1e-12 max|G| absolute, with saturated, zero, negative-zero and tiny outputs.
Operator level: GAT(..., activation=("elu", "identity")) on 15d_fusion2, c = 1 over loopback ranks against the numpy definition at 1e-10
(the bound of the additive operator tests) with and without dropout, with score dot in both backward modes, at the benchmark widths and
on an R-MAT graph with hub rows; refusals; the all-relu default bit for bit; a training run of the published layers.

Every test prints its observed error before it asserts and records the worst case with T.record_observed.  Observed on an MI355X
(profiles/gat_activation_gputests.log): the forward finish at most 2.1e-14 (additive), 2.9e-14 (with dropout) and 3.7e-14 (dot-product softmax)
on the output and 1.9e-15 on lse; the dense helper at most 1.7e-14 max|G| (delta, identity, f = 256; dZ at most 1.3e-16); the operator at most 4.9e-15 without dropout (benchmark
widths) and 2.0e-14 with it; the 10-step trajectory 9.9e-16 in the parameters (bound 4.1e-9) and 3.1e-16 in the loss (bound 5.2e-11); the
training loss 1.418 -> 0.046 over LEARN_STEPS, held-out accuracy 0.988.  The operator's inputs are scaled so that every hidden layer's
aggregates reach below -0.5 on a quarter of the units at least (assert_hidden_is_signed)."""
import ctypes as C

import numpy as np
import pytest

import gat_gpu_harness as G
import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import (ALPHA, FWD, GROUPINGS, DropProblem, Problem, assembled, ctx, er8, hip_backend, one_round, same, setup,  # noqa: F401
                             softmax_pass, square_graph, teardown)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FTOL = 1e-12   # forward finish and the dense helper, absolute
MODE = dict(attention="softmax", score="additive")
BITS = {"relu": 0, "elu": K.ATTN_ACT_ELU, "identity": K.ATTN_ACT_IDENTITY}
ERR_INVALID = 1
M_ROWS, N_COLS = 300, 800
WIDTHS = [1, 7, 64, 100, 128, 256]


def short_degrees(seed, m=M_ROWS):
    """0 .. 16 nonzeros per row, some rows empty, a fifth with one (their aggregate is the gathered row itself: the whole range)"""
    d = np.random.default_rng(seed).integers(0, 17, m)
    d[::11] = 0
    d[1::5] = 1
    d[2] = 16
    return d


# ------------------------------------------------------------------------------------------------ forward finish: the additive entry points
class ActMixin:
    """The sibling Problem classes with the activation bits ORed into every finishing call, and gathered values in [-50, 5]."""
    act = "relu"

    def spread(self):
        f = self.f
        self.y[:, :f] = self.y[:, :f] * 27.5 - 22.5  # ([-1, 1] -> [-50, 5]; the scores' columns stay as they are)
        self.d["y"].set(self.y)
        return self

    def fn(self):
        real = super().fn()
        return lambda h, blk, a, flags, win, stream: real(h, blk, a, flags | (BITS[self.act] if flags & K.ATTN_FINISH else 0), win, stream)


class AddAct(ActMixin, Problem):
    pass


class DropAct(ActMixin, DropProblem):
    pass


def make(ctx, kind, f, odd=False, seed=0):
    cls = AddAct if kind == "add" else DropAct
    return cls(ctx, FWD, f, m=M_ROWS, ncols=N_COLS, seed=seed, odd=odd, degrees=short_degrees(f + seed)).spread()


def abs_err(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble) - want)))


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("kind", ["add", "drop"])
def test_additive_finish_vs_extended_reference(ctx, kind, f, odd):
    p = make(ctx, kind, f, odd)
    o, lse = p.raw()
    assert o.min() < -30 and o.max() > 1, "the aggregates span the activation's two sides"
    res = {}
    for act in ("relu", "elu", "identity"):
        p.act = act
        res[act] = p.run(True)  # (asserts the guards)
        want = R.act_ld(o, act)
        errs = (abs_err(res[act]["out"], want), abs_err(res[act]["lse"], lse))
        T.record_observed("gat_activation_kernel", case="%s f=%d%s %s" % (kind, f, " odd" if odd else "", act), worst=max(errs))
        print("observed", kind, f, odd, act, "out %.2e lse %.2e" % errs)
        assert max(errs) <= FTOL and not np.any(np.isnan(res[act]["out"]))
        assert same(p.run(True), res[act]), "a repeat must be bit-identical"
    for act in ("elu", "identity"):
        assert np.count_nonzero(res[act]["out"] < 0) >= res[act]["out"].size // 4, "at least a quarter of the outputs are negative"
        assert np.array_equal(res[act]["lse"], res["relu"]["lse"]) and np.array_equal(res[act]["state"], res["relu"]["state"])
    # the ReLU default: the same call's identity output through max(., 0), bit for bit
    assert np.array_equal(res["relu"]["out"], np.maximum(res["identity"]["out"], 0.0))
    deg = np.diff(p.rowptr)
    assert all(np.all(res[a]["out"][deg == 0] == 0.0) for a in res), "a row without nonzeros: out = 0 under every activation"
    p.free()


@pytest.mark.parametrize("f", [7, 128, 256])
@pytest.mark.parametrize("kind", ["add", "drop"])
def test_additive_grouping_independence(ctx, kind, f):
    p = make(ctx, kind, f, seed=3)
    p.act = "elu"
    whole = p.run(True)
    for name, groups in GROUPINGS.items():
        assert same(p.run(True, groups), whole), name
    p.free()


@pytest.mark.parametrize("kind", ["add", "drop"])
def test_additive_empty_blocks(ctx, kind):
    """rowptr == NULL resets and finishes to zeros; it finishes a state left by an earlier call to the whole pass's bits; a block whose rows
    have no nonzeros (rowptr given) does the same through the row kernel."""
    f = 33
    p = make(ctx, kind, f)
    p.act = "elu"
    whole = p.run(True)
    a, blk = p.args(), p.block()
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    bits = K.ATTN_ACT_ELU
    call = Problem.fn(p) if kind == "add" else DropProblem.fn(p)  # the entry point without the mixin's bits

    def outputs():
        ctx.sync()
        out, state = p.d["out"].get(), p.d["state"].get()
        return out[:p.m, p.col0:p.col0 + f], state[2, :p.m], state[:2, :p.m], out

    for k, v in (("out", p.out0), ("state", p.state0), ("acc", p.acc0)):
        p.d[k].set(v)
    ctx.check(call(ctx.h, C.byref(none), C.byref(a), K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH | bits, None, K.STREAM_COMPUTE), "empty block, reset and finish")
    out, lse, state, full = outputs()
    assert np.all(out == 0.0) and np.all(lse == 0.0) and np.all(np.isneginf(state[0])) and np.all(state[1] == 0.0)
    assert np.array_equal(full[:, p.col0 + f:], p.out0[:, p.col0 + f:]) and np.array_equal(full[p.m], p.out0[p.m])
    # the nonzeros without a finish, then a block without nonzeros finishes the rows
    for k, v in (("out", p.out0), ("state", p.state0), ("acc", p.acc0)):
        p.d[k].set(v)
    ctx.check(call(ctx.h, C.byref(blk), C.byref(a), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE), "the nonzeros")
    ctx.check(call(ctx.h, C.byref(none), C.byref(a), K.ATTN_FINISH | bits, None, K.STREAM_COMPUTE), "empty block, finish")
    out, lse, state, _ = outputs()
    assert np.array_equal(out, whole["out"]) and np.array_equal(lse, whole["lse"]) and np.array_equal(state, whole["state"])
    assert np.count_nonzero(out < 0) > out.size // 4
    p.free()
    # a block with a rowptr whose rows are all empty
    q = (AddAct if kind == "add" else DropAct)(ctx, FWD, f, m=M_ROWS, ncols=N_COLS, degrees=np.concatenate([[2], np.zeros(M_ROWS - 1, dtype=np.int64)]))
    q.act = "elu"
    r = q.run(True)
    assert np.all(r["out"][1:] == 0.0) and np.all(r["lse"][1:] == 0.0) and np.all(np.isneginf(r["state"][0][1:])) and np.all(r["state"][1][1:] == 0.0)
    q.free()


@pytest.mark.parametrize("kind", ["add", "drop"])
def test_additive_flag_misuse_writes_nothing(ctx, kind):
    p = make(ctx, kind, 64)
    a, blk = p.args(), p.block()
    none = K.CsrBlock(p.m, 0, -1, 0, 0, None, None, None)
    call = Problem.fn(p) if kind == "add" else DropProblem.fn(p)
    ov, fin, elu, idn = K.FUSED_OUT_OVERWRITE, K.ATTN_FINISH, K.ATTN_ACT_ELU, K.ATTN_ACT_IDENTITY
    for k, v in (("out", p.out0), ("state", p.state0), ("acc", p.acc0), ("vec", p.vec0)):
        p.d[k].set(v)
    for b in (blk, none):
        for flags in (ov | fin | elu | idn, ov | elu, ov | idn, elu, idn, elu | idn):
            assert call(ctx.h, C.byref(b), C.byref(a), flags, None, K.STREAM_COMPUTE) == ERR_INVALID, flags
            assert b"HNH_ATTN" in ctx.lib.hnh_last_error(ctx.h)
    ctx.sync()
    assert np.array_equal(p.d["out"].get(), p.out0) and np.array_equal(p.d["state"].get(), p.state0) and np.array_equal(p.d["acc"].get(), p.acc0)
    # the backward passes take no activation bit at all
    for fn in ((ctx.lib.hnh_attn_add_row_csr_p, ctx.lib.hnh_attn_add_col_csr_p) if kind == "add" else ()):
        assert fn(ctx.h, C.byref(blk), C.byref(a), ov | elu, None, K.STREAM_COMPUTE) == ERR_INVALID
    p.free()


# ------------------------------------------------------------------------------------------------ forward finish: the dot-product softmax
class ActLib:
    """ctx.lib with the activation bits ORed into every finishing hnh_attn_softmax_csr_p call"""

    def __init__(self, lib, bits):
        self._lib, self._bits = lib, bits

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def hnh_attn_softmax_csr_p(self, h, blk, vals, x, y, out, r, flags, st, win, stream):
        return self._lib.hnh_attn_softmax_csr_p(h, blk, vals, x, y, out, r, flags | (self._bits if flags & K.ATTN_FINISH else 0), st, win, stream)


class ActCtx:
    def __init__(self, ctx, act):
        self._ctx, self.lib = ctx, ActLib(ctx.lib, BITS[act])

    def __getattr__(self, name):
        return getattr(self._ctx, name)


def softmax_problem(f, seed=0):
    m = M_ROWS
    rowptr, colidx, rows = square_graph(m, short_degrees(f + seed), f + seed + 1)
    rng = np.random.default_rng(50 * f + seed)
    x = rng.uniform(-1, 1, (m, f)) * 0.2 / np.sqrt(f)  # scores of a few units
    y = rng.uniform(-1, 1, (m, f)) * 27.5 - 22.5       # gathered values in [-50, 5]
    return rowptr, colidx, rows, x, y


# (a width above 256 needs the 16-byte instances, hnh_attention.h: 384 has no odd-offset case)
SOFTMAX_CASES = [(f, off) for f in WIDTHS for off in (2, 3)] + [(384, 2)]


@pytest.mark.parametrize("f,off", SOFTMAX_CASES, ids=["f%d%s" % (f, "_odd-offset" if off % 2 else "") for f, off in SOFTMAX_CASES])
def test_softmax_finish_vs_extended_reference(ctx, f, off):
    rowptr, colidx, rows, x, y = softmax_problem(f)
    o, lse, _ = P.attention_ld(rows, colidx.astype(np.int64), M_ROWS, x, y, ALPHA)
    assert o.min() < -30 and o.max() > 1
    res = {}
    for act in ("relu", "elu", "identity"):
        res[act] = softmax_pass(ActCtx(ctx, act), rowptr, colidx, x, y, ALPHA, off=off)  # (asserts the columns outside the head's block)
        errs = (abs_err(res[act][0], R.act_ld(o, act)), abs_err(res[act][1], lse))
        T.record_observed("gat_activation_kernel", case="softmax f=%d off=%d %s" % (f, off, act), worst=max(errs))
        print("observed softmax", f, off, act, "out %.2e lse %.2e" % errs)
        assert max(errs) <= FTOL and not np.any(np.isnan(res[act][0]))
        again = softmax_pass(ActCtx(ctx, act), rowptr, colidx, x, y, ALPHA, off=off)
        assert all(np.array_equal(a, b) for a, b in zip(res[act], again)), "two calls must be bit-identical"
    for act in ("elu", "identity"):
        assert np.count_nonzero(res[act][0] < 0) >= res[act][0].size // 4
        assert all(np.array_equal(a, b) for a, b in zip(res[act][1:], res["relu"][1:])), "lse, the row state and the scores do not depend on the activation"
    assert np.array_equal(res["relu"][0], np.maximum(res["identity"][0], 0.0))
    plain = softmax_pass(ctx, rowptr, colidx, x, y, ALPHA, off=off)
    assert all(np.array_equal(a, b) for a, b in zip(plain, res["relu"]))
    assert np.all(res["elu"][0][np.diff(rowptr) == 0] == 0.0)


@pytest.mark.parametrize("f", [7, 128, 256])
def test_softmax_grouping_independence(ctx, f):
    rowptr, colidx, rows, x, y = softmax_problem(f, seed=3)
    actx = ActCtx(ctx, "elu")
    whole = softmax_pass(actx, rowptr, colidx, x, y, ALPHA)
    for groups in GROUPINGS.values():
        if groups is not None:
            got = softmax_pass(actx, rowptr, colidx, x, y, ALPHA, groups=groups)
            assert all(np.array_equal(a, b) for a, b in zip(got, whole)), groups


def test_softmax_empty_block_and_flag_misuse(ctx):
    """rowptr == NULL as test_attention_instances_gpu.py::test_empty_block has it, with ELU and the identity on the finish; the refused flag
    combinations leave the sentinels."""
    lib, m, width, off = ctx.lib, 500, 100, 2
    ld = width + 4
    rng = np.random.default_rng(width)
    mx0, l0, out0 = rng.uniform(-3, 3, m), rng.uniform(0.5, 4.0, m), rng.uniform(-60, 8, (m, width))
    l0[::9], mx0[::9], out0[::9] = 0.0, -np.inf, 0.0
    none = K.CsrBlock(m, 0, -1, 0, 0, None, None, None)

    def call(flags, expect=0):
        d = dict(out=ctx.upload(out0), dst=ctx.upload(np.full((m, ld), 7.0)), lse=ctx.upload(np.full(m, 5.0)), rmax=ctx.upload(mx0), rsum=ctx.upload(l0))
        st = K.AttnState(d["rmax"].ptr, d["rsum"].ptr, d["lse"].ptr, ALPHA, d["dst"].ptr + off * 8, ld)
        rc = lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(none), None, None, None, d["out"].ptr, width, flags, C.byref(st), None, K.STREAM_COMPUTE)
        assert rc == expect, (flags, rc)
        ctx.sync()
        res = {k: v.get() for k, v in d.items()}
        for v in d.values():
            v.free()
        assert np.all(res["dst"][:, :off] == 7.0) and np.all(res["dst"][:, off + width:] == 7.0)
        res["dst"] = res["dst"][:, off:off + width]
        return res

    live = l0 > 0
    lse = np.zeros(m)
    lse[live] = mx0[live] + np.log(l0[live])
    for act in ("elu", "identity"):
        r = call(K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH | BITS[act])  # reset and finish: every row without nonzeros
        assert np.all(r["rmax"] == -np.inf) and np.all(r["rsum"] == 0.0) and np.all(r["dst"] == 0.0) and np.all(r["lse"] == 0.0)
        r = call(K.ATTN_FINISH | BITS[act])  # continue and finish
        want = np.zeros((m, width), dtype=np.longdouble)
        want[live] = R.act_ld(out0[live].astype(np.longdouble) / l0[live, None].astype(np.longdouble), act)
        assert np.array_equal(r["rmax"], mx0) and np.array_equal(r["rsum"], l0)
        assert abs_err(r["dst"], want) <= FTOL and np.all(r["dst"][~live] == 0.0) and np.count_nonzero(r["dst"] < 0) > r["dst"].size // 4
        assert np.all(np.abs(r["lse"] - lse) <= 1e-15 * np.maximum(1.0, np.abs(lse)))
    ov, fin, elu, idn = K.FUSED_OUT_OVERWRITE, K.ATTN_FINISH, K.ATTN_ACT_ELU, K.ATTN_ACT_IDENTITY
    for flags in (ov | fin | elu | idn, ov | elu, idn, elu | idn):
        r = call(flags, expect=ERR_INVALID)
        assert np.all(r["dst"] == 7.0) and np.all(r["lse"] == 5.0) and np.array_equal(r["rmax"], mx0) and np.array_equal(r["rsum"], l0)
        assert np.array_equal(r["out"].reshape(m, width), out0)


def test_softmax_real_block_flag_misuse_and_empty_finishing_rows(ctx):
    """The refused flag combinations on blocks with nonzeros leave every destination as it was.  Then the pass in two blocks: every row's
    nonzeros but row 2's in a call without a finish, and a finishing call over a block in which only row 2 has nonzeros, so that every
    other row is finished without a nonzero of its own in that call: the whole pass's bits."""
    lib, f, off = ctx.lib, 33, 3
    m, ld = M_ROWS, f + 4
    rowptr, colidx, rows, x, y = softmax_problem(f)
    assert rowptr[3] - rowptr[2] == 16
    nnz = int(rowptr[-1])
    whole = softmax_pass(ActCtx(ctx, "elu"), rowptr, colidx, x, y, ALPHA, off=off)
    deg = np.diff(rowptr)
    deg_a, deg_b = deg.copy(), np.zeros_like(deg)
    deg_a[2], deg_b[2] = 0, 16
    rp_a, rp_b = (np.concatenate([[0], np.cumsum(v)]).astype(np.int32) for v in (deg_a, deg_b))
    ci_a = np.concatenate([colidx[:rowptr[2]], colidx[rowptr[3]:], [0]]).astype(np.int32)
    ci_b = np.concatenate([colidx[rowptr[2]:rowptr[3]], [0]]).astype(np.int32)
    out0, vals0, dst0 = np.full(m * f, 2.0), np.full(nnz, 3.0), np.full((m, ld), 7.0)
    d = dict(rp_a=ctx.upload(rp_a), ci_a=ctx.upload(ci_a), rp_b=ctx.upload(rp_b), ci_b=ctx.upload(ci_b), x=ctx.upload(x), y=ctx.upload(y),
             out=ctx.upload(out0), vals=ctx.upload(vals0), rmax=ctx.upload(np.full(m, 5.0)), rsum=ctx.upload(np.full(m, 5.0)),
             lse=ctx.upload(np.full(m, 5.0)), dst=ctx.upload(dst0))
    blk_a = K.CsrBlock(m, nnz - 16, m, int(deg_a.max()), 0, d["rp_a"].ptr, d["ci_a"].ptr, None)
    blk_b = K.CsrBlock(m, 16, m, 16, 0, d["rp_b"].ptr, d["ci_b"].ptr, None)
    st = K.AttnState(d["rmax"].ptr, d["rsum"].ptr, d["lse"].ptr, ALPHA, d["dst"].ptr + off * 8, ld)

    def call(b, flags):
        return lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(b), d["vals"].ptr, d["x"].ptr, d["y"].ptr, d["out"].ptr, f, flags, C.byref(st), None, K.STREAM_COMPUTE)

    vo, ov, fin, elu, idn = K.FUSED_VALUES_OVERWRITE, K.FUSED_OUT_OVERWRITE, K.ATTN_FINISH, K.ATTN_ACT_ELU, K.ATTN_ACT_IDENTITY
    for b in (blk_a, blk_b):
        for flags in (vo | ov | fin | elu | idn, vo | ov | elu, vo | ov | idn, elu, idn, elu | idn):
            assert call(b, flags) == ERR_INVALID, flags
            assert b"HNH_ATTN" in lib.hnh_last_error(ctx.h)
    ctx.sync()
    assert np.array_equal(d["dst"].get(), dst0) and np.array_equal(d["out"].get(), out0) and np.array_equal(d["vals"].get(), vals0)
    assert all(np.all(d[k].get() == 5.0) for k in ("rmax", "rsum", "lse"))
    ctx.check(call(blk_a, vo | ov), "every row's nonzeros but row 2's")
    ctx.check(call(blk_b, vo | fin | elu), "row 2's nonzeros and the finish of every row")
    ctx.sync()
    dst = d["dst"].get()
    assert np.all(dst[:, :off] == 7.0) and np.all(dst[:, off + f:] == 7.0)
    got = (dst[:, off:off + f], d["lse"].get(), d["rmax"].get(), d["rsum"].get())
    assert all(np.array_equal(a, b) for a, b in zip(got, whole))
    assert np.count_nonzero(got[0] < 0) >= got[0].size // 4
    for v in d.values():
        v.free()


# ------------------------------------------------------------------------------------------------ hnh_act_grad_cols_f64
def act_grad_case(ctx, rows, f, act, even):
    """Three heads of f columns in G and out (the middle one is the call's), dZ at its own pitch with guard columns, delta with guards.
    even = 1: every pitch and offset even (16-byte lanes when f is even); 0: odd pitches; 2: even pitches and offsets, but dZ starts 8
    bytes off a 16-byte boundary (8-byte lanes by the base alone)."""
    lib = ctx.lib
    rng = np.random.default_rng(1000 * rows + 10 * f + even)
    skew, even = (1, 1) if even == 2 else (0, even)
    col0 = f + (f & 1) if even else f
    ld_g, ld_o, ld_dz = 3 * f + 4, 3 * f + 6, f + 2
    ld_g, ld_o, ld_dz = (v + (v % 2 if even else 1 - v % 2) for v in (ld_g, ld_o, ld_dz))
    assert all(v % 2 == (0 if even else 1) for v in (ld_g, ld_o, ld_dz)) and (not even or col0 % 2 == 0)
    g = rng.uniform(-3, 3, (rows, ld_g))
    # the bound is absolute (1e-12 max|G|), so the stored values' scale is chosen for it: delta sums f terms of at most max|G| max|o|, and
    # 256 * 8 * 2^-53 = 2.3e-13.  ELU (saturating below -37) and ReLU store at most 4 in magnitude; the identity stores o itself: the
    # forward tests' whole range [-50, 5] up to f = 7 (at most 4 roundings of a sum of 7 * 50 max|G|: 1.6e-13 max|G|), [-8, 4] above
    o = rng.uniform(-40, 4, (rows, ld_o)) if act != "identity" else (rng.uniform(-50, 5, (rows, ld_o)) if f <= 7 else rng.uniform(-8, 4, (rows, ld_o)))
    out = R.act(o, "elu") if act == "elu" else (np.maximum(o, 0) if act == "relu" else o.copy())
    special = np.array([-1.0, 0.0, -0.0, -1.0 + 2.0 ** -53, -1e-300, 1e-300, -5e-324, -1e-17, 1e-17, -0.999999999999])
    flat = out[:, col0:col0 + f].reshape(-1)
    idx = rng.permutation(flat.size)[:min(flat.size, len(special))]
    flat[idx] = special[:len(idx)] if act != "relu" else np.abs(special[:len(idx)])
    out[:, col0:col0 + f] = flat.reshape(rows, f)
    dz0, dl0 = np.full((rows + 1) * ld_dz + skew, 7.0), np.full(rows + 2, 9.0)  # (dZ begins `skew` doubles into its buffer)
    d = dict(g=ctx.upload(g), out=ctx.upload(out), dz=ctx.upload(dz0), dl=ctx.upload(dl0))
    assert d["dz"].ptr % 16 == 0 and d["g"].ptr % 16 == 0 and d["out"].ptr % 16 == 0

    def run():
        d["dz"].set(dz0)
        d["dl"].set(dl0)
        ctx.check(lib.hnh_act_grad_cols_f64(ctx.h, d["dz"].ptr + 8 * skew, ld_dz, d["dl"].ptr + 8, d["g"].ptr, ld_g, d["out"].ptr, ld_o, col0, rows, f,
                                            R.ACT_CODE[act], K.STREAM_COMPUTE), "hnh_act_grad_cols_f64")
        ctx.sync()
        flat = d["dz"].get().reshape(-1)
        assert np.all(flat[:skew] == 7.0)
        return flat[skew:].reshape(rows + 1, ld_dz), d["dl"].get()

    dz, dl = run()
    assert np.all(dz[:rows, f:] == 7.0) and np.all(dz[rows] == 7.0) and dl[0] == 9.0 and dl[rows + 1] == 9.0, "guards"
    assert not np.any(np.isnan(dz[:rows, :f])) and not np.any(np.isnan(dl[1:rows + 1]))
    want_dz, want_dl = R.stored_grad_ld(g[:, col0:col0 + f], out[:, col0:col0 + f], act)
    gmax = np.abs(g).max()
    errs = (abs_err(dz[:rows, :f], want_dz) / gmax, abs_err(dl[1:rows + 1], want_dl) / gmax)
    dz2, dl2 = run()
    assert np.array_equal(dz, dz2) and np.array_equal(dl, dl2), "a second run must be bit-identical"
    if act == "relu":
        d["dz"].set(dz0)
        ctx.check(lib.hnh_relu_grad_cols_f64(ctx.h, d["dz"].ptr + 8 * skew, ld_dz, d["g"].ptr, ld_g, d["out"].ptr, ld_o, col0, rows, f, K.STREAM_COMPUTE),
                  "relu_grad")
        ctx.sync()
        assert np.array_equal(d["dz"].get().reshape(-1)[skew:].reshape(rows + 1, ld_dz), dz), "act = relu is hnh_relu_grad_cols_f64's dZ bit for bit"
    if act == "elu":
        sat = out[:, col0:col0 + f] == -1.0
        assert np.all(dz[:rows, :f][sat] == 0.0)
    for v in d.values():
        v.free()
    return errs


@pytest.mark.parametrize("even", [1, 0, 2], ids=["even-pitches", "odd-pitches", "even-pitches-odd-base"])
@pytest.mark.parametrize("f", [1, 3, 7, 64, 100, 256])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_act_grad_cols_vs_extended_reference(ctx, rows, f, even):
    worst = {}
    for act in R.ACTIVATIONS:
        worst[act] = act_grad_case(ctx, rows, f, act, even)
    T.record_observed("gat_activation_act_grad", case="rows=%d f=%d even=%d" % (rows, f, even), worst=max(max(v) for v in worst.values()))
    print("observed act_grad", rows, f, even, {k: "dZ %.2e delta %.2e" % v for k, v in worst.items()})
    # the delta of a row sums f terms of size <= max|G| max(|o|, 1): 1e-12 max|G| per the issue; f = 256 terms of 40 each stay far inside
    assert all(max(v) <= FTOL for v in worst.values()), worst


def test_act_grad_cols_argument_checks(ctx):
    lib = ctx.lib
    buf = ctx.upload(np.full(64, 7.0))
    p = buf.ptr

    def call(dz=p, ld_dz=4, dl=p, g=p, ld_g=8, out=p, ld_o=8, col0=2, rows=2, cols=4, act=1):
        return lib.hnh_act_grad_cols_f64(ctx.h, dz, ld_dz, dl, g, ld_g, out, ld_o, col0, rows, cols, act, K.STREAM_COMPUTE)

    for kw in (dict(dz=None), dict(dl=None), dict(g=None), dict(out=None), dict(rows=-1), dict(cols=-1), dict(col0=-1), dict(col0=5), dict(ld_dz=3),
               dict(ld_g=5), dict(ld_o=5), dict(act=3), dict(act=-1)):
        assert call(**kw) == ERR_INVALID, kw
        assert b"hnh_act_grad_cols_f64" in lib.hnh_last_error(ctx.h)
    assert call(rows=0) == 0
    ctx.sync()
    assert np.all(buf.get() == 7.0), "refused and empty calls write nothing"
    buf.free()


# ------------------------------------------------------------------------------------------------ the operator
ACTS = ("elu", "identity")
LAYERS = [(24, 16, 2), (32, 7, 3)]


def signed_parameters(layers, seed=13, scale=2.0):
    """W of scale / sqrt(fan-in), a1 and a2 of order one: aggregates of order one on both sides of 0"""
    rng = np.random.default_rng(seed)
    w = {(li, h): rng.standard_normal((fin, fph)) * scale / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    return w, R.vectors_of(layers, seed=seed + 1)


def run_case(world, rows, cols, m, x, layers, w, av, g, additive=True, **kw):
    return G.run_rounds(world, rows, cols, m, x, layers, w, av if additive else None, g, attention="softmax", score="additive" if additive else "dot", **kw)


def compare(got, want, label, ranks):
    G.compare(got, want, "gat_activation", label, ranks)


def reference(rows, cols, m, x, layers, w, av, g, acts=ACTS, rates=(0.0, 0.0), seed=0, score="additive"):
    return G.reference(rows, cols, m, x, layers, w, av, g, attention="softmax", score=score, rates=rates, seed=seed, activations=acts)


def er8_problem():
    rows, cols, m, _ = er8()
    x = O.dense_fill(m, LAYERS[0][0], 41) * 24.0  # (dense_fill is within 1/24: features of order one, hidden aggregates of a few units)
    w, av = signed_parameters(LAYERS)
    g = O.dense_fill(m, LAYERS[-1][1] * LAYERS[-1][2], 9) * 16.0
    return rows, cols, m, x, w, av, g


def assert_hidden_is_signed(rows, cols, m, x, layers, w, av, acts):
    """the inputs' own check: every hidden layer's aggregates are negative for a quarter of the units at least and reach below -0.5, so
    that ELU differs from the identity and from ReLU where the comparison looks"""
    pre = R.pre_activations(rows, cols, m, x, layers, ALPHA, w, av, activations=acts, **MODE)
    for li in range(len(layers) - 1):
        hidden = np.concatenate([o.reshape(-1) for _, o in pre[li]])
        assert np.count_nonzero(hidden < 0) >= hidden.size // 4 and hidden.min() < -0.5, "the hidden ELU of layer %d sees its negative side" % li


ER8 = {}


@pytest.mark.parametrize("p", [1, 2, 4, 8])
def test_operator_er8(p):
    rows, cols, m, x, w, av, g = er8_problem()
    if "ref" not in ER8:
        ER8["ref"] = reference(rows, cols, m, x, LAYERS, w, av, g)
        assert_hidden_is_signed(rows, cols, m, x, LAYERS, w, av, ACTS)
        assert ER8["ref"]["out"].min() < 0, "the identity output is signed"
    per_rank = H.run_spmd(p, lambda wd: run_case(wd, rows, cols, m, x, LAYERS, w, av, g, activation=ACTS))
    got = assembled(per_rank, 0, m, LAYERS)
    compare(got, ER8["ref"], "er8 elu/identity p%d" % p, p)
    ER8[p] = got


def test_one_rank_and_eight_ranks_agree():
    rows, cols, m, x, w, av, g = er8_problem()
    res = {p: ER8.get(p) or assembled(H.run_spmd(p, lambda wd: run_case(wd, rows, cols, m, x, LAYERS, w, av, g, activation=ACTS)), 0, m, LAYERS) for p in (1, 8)}
    compare(res[8], res[1], "er8 elu/identity p8 against p1", 8)


@pytest.mark.parametrize("p", [1, 4])
def test_operator_with_dropout(p):
    rows, cols, m, x, w, av, g = er8_problem()
    rates, seed = (0.6, 0.6), 11
    per_rank = H.run_spmd(p, lambda wd: run_case(wd, rows, cols, m, x, LAYERS, w, av, g, activation=ACTS, dropout=rates, seed=seed))
    compare(assembled(per_rank, 0, m, LAYERS), reference(rows, cols, m, x, LAYERS, w, av, g, rates=rates, seed=seed), "er8 dropout p%d" % p, p)


@pytest.mark.parametrize("backward", ["unfused", "fused"])
@pytest.mark.parametrize("p", [1, 4])
def test_operator_score_dot(p, backward):
    rows, cols, m, x, w, av, g = er8_problem()
    w = {k: v * 0.5 for k, v in w.items()}  # (dot-product scores are quadratic in W)
    per_rank = H.run_spmd(p, lambda wd: run_case(wd, rows, cols, m, x, LAYERS, w, None, g, additive=False, activation=ACTS, backward=backward))
    want = reference(rows, cols, m, x, LAYERS, w, None, g, score="dot")
    assert want["out"].min() < 0
    compare(assembled(per_rank, 0, m, LAYERS), want, "er8 dot %s p%d" % (backward, p), p)


def test_operator_benchmark_widths():
    m, layers = 1 << 12, [(256, 256, 1), (256, 128, 2), (256, 64, 3)]
    rows, cols = H.generate_er(m, m, m * 16, 77)
    x = O.dense_fill(m, 256, 41) * 24.0
    w, av = signed_parameters(layers, seed=5, scale=6.0)  # (a mean over 16 neighbours shrinks each layer's values fourfold)
    g = O.dense_fill(m, 192, 3) * 64.0
    acts = ("elu", "elu", "identity")
    assert_hidden_is_signed(rows, cols, m, x, layers, w, av, acts)
    per_rank = H.run_spmd(1, lambda wd: run_case(wd, rows, cols, m, x, layers, w, av, g, activation=acts))
    ref = reference(rows, cols, m, x, layers, w, av, g, acts=acts)
    assert ref["out"].min() < 0
    compare(assembled(per_rank, 0, m, layers), ref, "benchmark widths", 1)


def test_operator_rmat_hub_rows():
    m, layers = 1 << 13, [(64, 64, 2), (128, 32, 2)]
    rows, cols = H.generate_rmat(13, m * 16)
    assert np.bincount(rows, minlength=m).max() >= 512 and np.bincount(cols, minlength=m).max() >= 512
    x = O.dense_fill(m, 64, 8) * 24.0
    w, av = signed_parameters(layers, seed=6, scale=2.0)
    g = O.dense_fill(m, 64, 4) * 32.0
    assert_hidden_is_signed(rows, cols, m, x, layers, w, av, ACTS)
    per_rank = H.run_spmd(1, lambda wd: run_case(wd, rows, cols, m, x, layers, w, av, g, activation=ACTS))
    compare(assembled(per_rank, 0, m, layers), reference(rows, cols, m, x, layers, w, av, g), "rmat hubs", 1)


@pytest.mark.parametrize("alg,attention,words", [("15d_fusion2", "none", "attention mode softmax only"), ("15d_fusion1", "softmax", "15d_fusion1.*c = 1")])
def test_refusals_leave_nothing_in_flight(alg, attention, words):
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    words = "activation elu of layer 0.*" + words

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
        d = H.DistributedSparse(world, alg, sp, 16, 1)
        gnn = H.GAT(d, layers, ALPHA, attention=attention, activation=("elu", "relu"))
        for k in [(li, h) for li, (_, _, heads) in enumerate(layers) for h in range(heads)]:
            gnn.set_weight(*k, O.gat_weight(k[0], k[1], layers[k[0]][0], layers[k[0]][1]))
        g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
        with pytest.raises(H.HnhError, match=words):
            gnn.forwardPass()
        with pytest.raises(H.HnhError, match=words):
            gnn.backwardPass(g)
        if alg == "15d_fusion2":  # (train_step and evaluate on 15d_fusion1 are refused for the loss's own reason first)
            gnn.set_labels(np.arange(m) % layers[-1][1], None, heads="mean")
            gnn.set_optimizer("adam", 0.01)
            for call in (gnn.train_step, gnn.evaluate):
                with pytest.raises(H.HnhError, match=words):
                    call()
        world.sync()  # nothing was left in flight
        with pytest.raises(ValueError):
            gnn.set_activation(0, "gelu")
        assert H.lib().hnh_gat_set_activation(gnn.h, 0, 7) != 0
        gnn.set_activation(0, "relu")  # the object runs normally afterwards
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


@pytest.mark.parametrize("p", [1, 4])
def test_default_is_untouched(p):
    """activation="relu" spelled out, an object switched to elu and back, and an object that never heard of the option: the same bits,
    output and gradients."""
    rows, cols, m, x = er8()
    layers = T.GAT_LAYERS
    w = {(li, h): O.gat_weight(li, h, fin, fph) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}
    av = R.vectors_of(layers)
    g = O.dense_fill(m, 12, 9) * 16.0

    def plain(world):
        return run_case(world, rows, cols, m, x, layers, w, av, g)["rounds"][0]

    def spelled(world):
        return run_case(world, rows, cols, m, x, layers, w, av, g, activation="relu")["rounds"][0]

    def trip(world):
        s = setup(world, rows, cols, m, x, layers, w, av, g, attention="softmax", score="additive")
        s["gnn"].forwardPass()
        s["gnn"].set_activation(0, "elu")
        with pytest.raises(H.HnhError, match="forwardPass"):
            s["gnn"].backwardPass(s["g"])  # a change of activation invalidates the stored forward pass
        mid = one_round(s, w, True)
        s["gnn"].set_activation(0, "relu")
        after = one_round(s, w, True)
        teardown(s)
        return mid, after

    for old, named, (mid, after) in zip(H.run_spmd(p, plain), H.run_spmd(p, spelled), H.run_spmd(p, trip)):
        for a in (named, after):
            assert np.array_equal(old["out"], a["out"]) and np.array_equal(old["dx"], a["dx"])
            assert all(np.array_equal(old["dw"][k], a["dw"][k]) and np.array_equal(old["da"][k][0], a["da"][k][0]) and
                       np.array_equal(old["da"][k][1], a["da"][k][1]) for k in w)
        assert not np.array_equal(mid["out"], old["out"]), "the elu round computed something else"


# ------------------------------------------------------------------------------------------------ training
def device_train(world, pp, layers, optimizer, steps):
    s = setup(world, pp["rows"], pp["cols"], pp["m"], pp["x"], layers, pp["w"], pp["av"], None, attention="softmax", score="additive", activation=ACTS)
    gnn = s["gnn"]
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
    res["held"] = gnn.evaluate(~pp["mask"])
    teardown(s)
    return res


@pytest.mark.parametrize("p", [1, 4])
def test_training_the_published_layers(p):
    """Hidden ELU, identity output, heads "mean" on gat_ref.planted_partition: the 10-step Adam trajectory within 10 x the divergence
    of a reference run whose gradients are perturbed by 1e-10 (the criterion of test_gat_train_gpu.py); after LEARN_STEPS the training loss
    is below its starting value; the parameters are bit-equal across the ranks."""
    layers = T.GAT_LAYERS
    pp = R.planted_partition(layers)
    opt = dict(kind="adam", lr=0.01, weight_decay=5e-4)
    args = (pp["rows"], pp["cols"], pp["m"], pp["x"], layers, ALPHA, pp["labels"], pp["mask"], "mean", pp["w"], pp["av"])
    ref = R.train(*args, opt, 10, activations=ACTS)
    per = R.train(*args, opt, 10, activations=ACTS, perturb=(1e-10, np.random.default_rng(7)))
    bound_p = 10.0 * R.parameter_divergence(per[2], per[3], ref[2], ref[3])
    bound_l = 10.0 * float(np.max(np.abs(np.array(per[0]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    assert bound_p > 0 and bound_l > 0
    per_rank = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, opt, 10))
    r0 = per_rank[0]
    for pr in per_rank:
        assert pr["losses"] == r0["losses"] and pr["accs"] == r0["accs"]
        for k in r0["w"]:
            assert np.array_equal(pr["w"][k], r0["w"][k]), "parameters are bit-equal across ranks"
            assert np.array_equal(pr["av"][k][0], r0["av"][k][0]) and np.array_equal(pr["av"][k][1], r0["av"][k][1])
    got_p = R.parameter_divergence(r0["w"], r0["av"], ref[2], ref[3])
    got_l = float(np.max(np.abs(np.array(r0["losses"]) - np.array(ref[0]))) / np.max(np.abs(ref[0])))
    T.record_observed("gat_activation_trajectory", ranks=p, parameters=got_p, parameters_bound=bound_p, loss=got_l, loss_bound=bound_l)
    print("observed trajectory", p, "parameters %.2e (bound %.2e) loss %.2e (bound %.2e)" % (got_p, bound_p, got_l, bound_l))
    assert got_p <= bound_p and got_l <= bound_l and r0["accs"] == ref[1]
    long_run = H.run_spmd(p, lambda wd: device_train(wd, pp, layers, R.LEARN_OPTIMIZER, R.LEARN_STEPS))
    lr0 = long_run[0]
    print("observed learning: loss %.3f -> %.3f, held-out accuracy %.3f" % (lr0["losses"][0], lr0["losses"][-1], lr0["held"][1]))
    assert lr0["losses"][-1] < lr0["losses"][0]
    assert all(np.array_equal(pr["w"][k], lr0["w"][k]) for pr in long_run for k in lr0["w"])
