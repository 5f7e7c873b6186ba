"""The dense kernels of the GAT's training path on the device, at every instance and past every grid cap: layer normalisation
(13 instances <W, T, BLOCK> of layernorm_fwd_kernel and of layernorm_bwd_kernel, every lane group of the wave shape, the cap of 1024 row
ranges), hnh_colsum_f64 (both widths, the cap of 512 ranges), hnh_act_grad_cols_f64 and hnh_skip_grad_cols_f64 (every lane group, the
trip loop), hnh_skip_addend_cols_f64 past ew_grid's cap, the optimizer steps past 1024 workgroups and hnh_grad_sumsq_f64 past 2048.

tests/train_dense_cases.py holds the design: the case tables, the dispatchers restated in Python, operands on which the result is exact
(compared by bit pattern against int64 / dyadic host models), NaN guards round every buffer of the new calls and NormCase's guards round
the norm's.  Only ELU, dz (its row means divide by cols) and Adam / AdamW are compared by distance, each against the reference and the
bound its own test file already uses: forward 32 eps64 (1 + max|z_r| / sigma_r) max(1, max|gamma|), dz 128 eps64 (1 + max|z_r| / sigma_r)
max|G| max|gamma| / sigma_r, the stored-output gradients 1e-12 max|G|, the optimizer T.TOL.  tests/test_train_dense_instances_cpu.py
checks the tables and the models themselves.

Every test prints its observed share of a bound before it asserts and records it with T.record_observed.  Observed on an MI355X
(profiles/train_dense_instances_gputests.log; the kernels launched: profiles/train_dense_instances_kernels.txt): every exact comparison
holds; the forward kernel at most 0.035 of its bound (33 columns, 8-byte lanes), dz 0.0088 (1024 columns, 8-byte lanes); on the exact
operands ELU's forward 0.0018 and dz 0.0050 of theirs, dz at the range caps 0.0052 (262 144 x 6); the ELU gradients of the two column
kernels 2.0e-15 max|G| against 1e-12; Adam and AdamW past the cap 2.7e-16 against T.TOL = 1e-11.  No kernel was found wrong."""
import numpy as np
import pytest

import hnh_testlib as T
import test_gat_activation_gpu as AG
import test_gat_norm_gpu as NG
import test_gat_skip_gpu as SG
import train_dense_cases as TD
from distributed_sddmm_amd import _kernels as K
from gat_gpu_harness import FTOL, ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. layer norm, every instance
@pytest.mark.parametrize("case", TD.NORM_CASES, ids=[TD.norm_id(c) for c in TD.NORM_CASES])
def test_layernorm_every_instance_vs_extended_reference(ctx, case):
    cols, odd = case
    worst = [0.0, 0.0]
    for rows, act, shift in TD.norm_runs(cols, odd):
        f, b = NG.check_case(ctx, rows, cols, act, shift, odd)
        worst = [max(worst[0], f), max(worst[1], b)]
    T.record_observed("train_dense_layernorm", case=TD.norm_id(case), instance=str(TD.norm_instance_of(cols, TD.norm_vec(cols, odd))), forward=worst[0],
                      backward=worst[1])
    print("observed layernorm", TD.norm_id(case), TD.norm_instance_of(cols, TD.norm_vec(cols, odd)), "forward %.3f of its bound, dz %.3f of its bound" % tuple(worst))


# ------------------------------------------------------------------------------------------------ 2. layer norm, exact
EVEN_NORM_CASES = [c for c in TD.NORM_CASES if c[0] % 2 == 0]


@pytest.mark.parametrize("case", EVEN_NORM_CASES, ids=[TD.norm_id(c) for c in EVEN_NORM_CASES])
def test_layernorm_exact(ctx, case):
    cols, odd = case
    rows = TD.norm_rows(cols, odd)
    worst = [0.0, 0.0]
    # the ragged count with rows of +-1 and every activation, the three ranges with rows of 3 +- 1, the counts below with one of the two
    for r, base, acts in ((rows[-2], 0.0, TD.ACTS3), (rows[-1], 3.0, TD.ACTS3), (rows[0], 3.0, TD.EXACT_ACTS), (rows[-3], 0.0, ("relu",))):
        f, b = TD.norm_exact(ctx, r, cols, odd, base, acts)
        worst = [max(worst[0], f), max(worst[1], b)]
    T.record_observed("train_dense_layernorm_exact", case=TD.norm_id(case), forward=worst[0], backward=worst[1])
    print("observed exact layernorm", TD.norm_id(case), "elu forward %.3f of its bound, dz %.3f of its bound" % tuple(worst))


# ------------------------------------------------------------------------------------------------ 3. the range caps, exact
@pytest.mark.parametrize("case", TD.NORM_CAPS, ids=["%dx%d%s" % (c[0], c[1], "_odd" if c[2] else "") for c in TD.NORM_CAPS])
def test_layernorm_range_caps_exact(ctx, case):
    rows, cols, odd, capped = case
    ranges, per = TD.norm_plan(rows, cols)
    assert (per > (TD.NORM_NARROW_ROWS if cols <= TD.NORM_NARROW else TD.NORM_WIDE_ROWS)) == capped
    f, b = TD.norm_exact(ctx, rows, cols, odd, 3.0 if cols > 6 else 0.0, ("relu",) if cols > 6 else TD.EXACT_ACTS, light=True)
    T.record_observed("train_dense_layernorm_caps", case="%dx%d odd=%s" % (rows, cols, odd), ranges=ranges, per=per, backward=b)
    print("observed layernorm at", rows, cols, odd, "ranges", ranges, "per", per, "dz %.3f of its bound" % b)


# ------------------------------------------------------------------------------------------------ 4. hnh_colsum_f64
@pytest.mark.parametrize("case", TD.COLSUM_CASES, ids=["%d%s" % (c[0], "_moved" if c[1] else "") for c in TD.COLSUM_CASES])
def test_colsum_exact(ctx, case):
    for rows in TD.COLSUM_ROWS:
        TD.colsum(ctx, rows, *case)


@pytest.mark.parametrize("case", TD.COLSUM_CAPS, ids=["%dx%d" % c[:2] for c in TD.COLSUM_CAPS])
def test_colsum_range_cap_exact(ctx, case):
    rows, cols, capped = case
    for moved in (False, True):
        TD.colsum(ctx, rows, cols, moved)


# ------------------------------------------------------------------------------------------------ 5. the two gradient kernels
@pytest.mark.parametrize("case", TD.GRAD_CASES, ids=[TD.grad_id(c) for c in TD.GRAD_CASES])
def test_act_grad_cols_exact(ctx, case):
    for rows in TD.grad_rows(*case):
        TD.act_grad(ctx, rows, *case)


@pytest.mark.parametrize("case", TD.GRAD_CASES, ids=[TD.grad_id(c) for c in TD.GRAD_CASES])
def test_skip_grad_cols_exact(ctx, case):
    for rows in TD.grad_rows(*case):
        TD.skip_grad(ctx, rows, *case)


@pytest.mark.parametrize("case", TD.GRAD_CASES, ids=[TD.grad_id(c) for c in TD.GRAD_CASES])
def test_grad_cols_elu_vs_extended_reference(ctx, case):
    """ELU through the siblings' cases (act_grad_case, skip_grad_case: guards, special values, repeats) at their bound, 1e-12 max|G|"""
    f, even = case
    worst = 0.0
    for rows in TD.grad_rows(f, even):
        errs = [AG.act_grad_case(ctx, rows, f, "elu", int(even))]
        errs += [SG.skip_grad_case(ctx, rows, f, "elu", int(even), res_kind, with_bias) for res_kind, with_bias in (("none", True), ("block", False), ("contiguous", True))]
        worst = max(worst, max(max(e) for e in errs))
        assert worst <= FTOL, (rows, errs)
    T.record_observed("train_dense_grad_cols_elu", case=TD.grad_id(case), worst=worst)
    print("observed elu gradients", TD.grad_id(case), "worst %.2e of max|G| (bound %.0e)" % (worst, FTOL))


# ------------------------------------------------------------------------------------------------ 6. hnh_skip_addend_cols_f64 past the cap
@pytest.mark.parametrize("case", list(TD.ADDEND_PAST), ids=[TD.addend_id(c) for c in TD.ADDEND_PAST])
def test_skip_addend_past_the_cap(ctx, case):
    TD.skip_addend(ctx, *case)


# ------------------------------------------------------------------------------------------------ 7. the optimizer steps past 1024 workgroups
def test_sgd_past_the_cap_exact(ctx):
    TD.optim_exact_sgd(ctx, "plain")


@pytest.mark.parametrize("coef", [1.0, 0.25])
def test_clipped_sgd_past_the_cap_exact(ctx, coef):
    TD.optim_exact_sgd(ctx, "clip", coef)


def test_adam_past_the_cap_vs_numpy(ctx):
    worst = TD.optim_adam(ctx)
    T.record_observed("train_dense_optim", case="adam", worst=worst)
    print("observed adam past the cap: worst %.2e (bound %.0e)" % (worst, T.TOL))
    assert worst <= T.TOL


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_clipped_adam_past_the_cap_vs_numpy(ctx, kind):
    worst = TD.optim_clip(ctx, kind)
    T.record_observed("train_dense_optim", case="clip " + kind, worst=worst)
    print("observed clipped", kind, "past the cap: worst %.2e (bound %.0e)" % (worst, T.TOL))
    assert worst <= T.TOL


# ------------------------------------------------------------------------------------------------ 8. hnh_grad_sumsq_f64 past 2048 workgroups
def test_sumsq_past_the_cap_alone(ctx):
    results = {}
    for name in TD.SUMSQ_BIG:
        g, entry, want = TD.sumsq_big(ctx, name)
        tab = (K.OptimTensor * 1)(entry)
        results[name] = TD.sumsq_checked(ctx, tab, 1, [g], want)
        assert TD.sumsq_checked(ctx, tab, 1, [g], want, accumulate=1, start=1234.5) == 1234.5 + want
        g.free()
    assert results["dense"] == results["dense_moved"], "16-byte and 8-byte loads: the same number"


def test_sumsq_past_the_cap_among_small_tensors(ctx):
    p, dev, small, parts = TD.sumsq_case(ctx, integer=True)
    want = int(sum(np.sum(np.square(a)) for a in parts))
    big = [TD.sumsq_big(ctx, name) for name in ("dense_moved", "pitched", "long_rows")]
    entries = list(small)
    tab = (K.OptimTensor * (len(entries) + 3))(*(entries[:10] + [big[0][1]] + entries[10:50] + [big[1][1]] + entries[50:] + [big[2][1]]))
    assert len(tab) == 66 > 2 * K.OPTIM_MAX_TENSORS
    total = want + sum(b[2] for b in big)
    guarded = [b[0] for b in big]
    assert TD.sumsq_checked(ctx, tab, len(tab), guarded, total) == float(total)
    TD.sumsq_checked(ctx, tab, len(tab), guarded, total, accumulate=1, start=0.5)
    for b in big:
        b[0].free()
    dev.free()
    p.free()
