"""tests/train_dense_cases.py without a GPU: the case tables of tests/test_train_dense_instances_gpu.py, the Python restatements of the
dispatchers and the exact host models themselves.  Every one of the 13 instances <W, T, BLOCK> of the two layernorm kernels and every
(W, lpr_log2) lane group of the three lane-group kernels is reached by the table; both sides of every switch point are in it; each
planned row count reaches its cap and its neighbour does not; the plans agree with the workspace functions of the device library (dlopen
needs no GPU); the exact models stay inside the bounds their exactness rests on.  A changed line of a restatement (the 512 of
norm_instance_of's block switch, a cap, a rounding of `per`) fails here.  The second CPU test double exports hnh_act_grad_cols_f64 and
hnh_optim_step_f64: those cases run on it too, under the stream-order checker, as tests/test_gat_double_cpu.py runs its list (the norm,
skip and clip groups are not in the double)."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as D
import gat_double_cases as DC
import hnh_testlib as T
import train_dense_cases as TD
from distributed_sddmm_amd import _kernels as K


# ------------------------------------------------------------------------------------------------ layer normalisation
def test_norm_table_reaches_every_instance_and_every_lane_group():
    assert set(TD.ISSUE_NORM_COLS) < set(TD.NORM_COLS) and len(TD.NORM_COLS) == len(TD.ISSUE_NORM_COLS) + 4
    assert len(TD.NORM_INSTANCES) == 13 == len(set(TD.NORM_INSTANCES))
    inst = {c: TD.norm_instance_of(c[0], TD.norm_vec(*c)) for c in TD.NORM_CASES}
    assert {v[:3] for v in inst.values()} == set(TD.NORM_INSTANCES), "both kernels take the same shape: 13 instances each"
    assert {(v[0], v[3]) for v in inst.values() if not v[2]} == {(w, l) for w in (1, 2) for l in range(7)}, "every (W, lpr_log2) of the wave shape"
    # the four instances and the ten groups that no earlier test launched
    assert inst[(258, False)][:3] == (2, 4, False) == inst[(512, False)][:3] and inst[(1026, False)][:3] == (2, 4, True) == inst[(2048, False)][:3]
    assert inst[(257, True)][:3] == (1, 2, True) == inst[(512, True)][:3] and inst[(1025, True)][:3] == (1, 8, True) == inst[(2048, True)][:3]
    want = {(3, True): (1, 2), (4, True): (1, 2), (16, True): (1, 4), (17, True): (1, 5), (32, True): (1, 5), (4, False): (2, 1), (8, False): (2, 2),
            (16, False): (2, 3), (32, False): (2, 4)}
    assert all((inst[c][0], inst[c][3]) == g and inst[c][1] == 1 for c, g in want.items())
    # every even width of the table runs both ways, so the exact operands (even widths) reach all 13 instances too
    even = {inst[c][:3] for c in TD.NORM_CASES if c[0] % 2 == 0}
    assert even == set(TD.NORM_INSTANCES) and {(inst[c][0], inst[c][3]) for c in TD.NORM_CASES if c[0] % 2 == 0 and not inst[c][2]} >= \
        {(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6)} | {(2, l) for l in range(7)}


def test_norm_instances_as_the_header_states_them():
    """norm_shape(): wave up to 64 W 4 columns, T the power of two that covers the row"""
    for w, vec in ((2, True), (1, False)):
        for cols in range(1, K.NORM_MAX_COLS + 1):
            if vec and cols % 2:
                continue
            ww, t, block, lpr = TD.norm_instance_of(cols, vec)
            lanes = 256 if block else 1 << lpr
            assert ww == w and block == (cols > 256 * w) and lanes * w * t >= cols and (t == 1 or lanes * w * t // 2 < cols)
            assert block or lpr == 6 or (lanes * w >= cols and (lpr == 0 or lanes * w // 2 < cols))
            assert (w, t, block) in TD.NORM_INSTANCES, (cols, w, t, block)


def test_norm_table_has_both_sides_of_every_switch():
    cases = set(TD.NORM_CASES)
    for w, pairs in TD.NORM_SWITCHES.items():
        for lo, hi in pairs:
            below, above = TD.norm_instance_of(lo, w == 2), TD.norm_instance_of(hi, w == 2)
            assert below[:3] != above[:3] and (w == 1 or TD.norm_instance_of(hi - 2, True) == below) and (w == 2 or hi == lo + 1)
            assert ((lo, w == 1) in cases or (w == 1 and lo % 2 == 0 and (lo, True) in cases)) and (hi, w == 1) in cases, (w, lo, hi)
    # the switch points of the issue, by name
    for trio in ((128, 130), (256, 257, 258), (512, 513, 514), (1024, 1025, 1026), (2048, 2049, 2050)):
        assert set(trio) <= set(TD.NORM_COLS)


def test_norm_rows_surround_a_workgroup_and_span_several_ranges():
    for cols, odd in TD.NORM_CASES:
        w, t, block, lpr = TD.norm_instance_of(cols, TD.norm_vec(cols, odd))
        rows = TD.norm_rows(cols, odd)
        groups = 1 if block else 256 >> lpr
        assert rows[:-1] == ([1, 2, 3] if block else [r for r in (groups - 1, groups, groups + 1) if r])
        assert TD.norm_plan(rows[-1], cols)[0] == 3 and all(TD.norm_plan(r, cols)[0] <= 2 for r in rows[:-1])
        runs = TD.norm_runs(cols, odd)
        assert {a for r, a, s in runs if r == rows[-2]} == set(TD.ACTS3) and {r for r, a, s in runs} == set(rows)
        assert any(s == 1000.0 for r, a, s in runs) and len(runs) <= 6


def test_norm_caps_and_their_neighbours():
    plans = {c[:2]: TD.norm_plan(*c[:2]) for c in TD.NORM_CAPS}
    assert plans[(17000, 514)] == (1000, 17) and plans[(16384, 514)] == (1024, 16)
    assert plans[(270001, 6)] == (1023, 264) and plans[(262144, 6)] == (1024, 256)
    for rows, cols, odd, capped in TD.NORM_CAPS:
        least = 256 if cols <= 512 else 16
        assert (-(-rows // least) > TD.NORM_RANGES) == capped and (TD.norm_plan(rows, cols)[1] > least) == capped
    assert TD.norm_plan(16385, 514) == (964, 17) and TD.norm_plan(262145, 6) == (1021, 257), "one row more is capped"
    hip = K.load()
    for rows, cols in list(plans) + [(1, 1), (257, 7), (600, 512), (37, 513), (5000, 768), (1 << 18, 3584), (16385, 514), (262145, 6), (255, 8), (513, 512)]:
        assert hip.hnh_layernorm_bwd_workspace(rows, cols) == TD.norm_plan(rows, cols)[0] * 2 * cols, (rows, cols)


def test_norm_exact_model_is_exact():
    for rows, cols, base in ((5, 4, 0.0), (5, 4, 3.0), (37, 514, 3.0), (270001, 6, 0.0)):
        z, gamma, beta, g, s = TD.norm_exact_operands(rows, cols, base)
        assert np.all(np.abs(s) == 1.0) and np.all(s.sum(axis=1) == 0.0) and set(np.unique(gamma)) <= {0.5, 1.0, 2.0}
        assert np.all(beta * 2 == np.rint(beta * 2)) and np.abs(beta).max() <= 2.0 and set(np.unique(g)) <= set(range(-4, 5))
        if rows > 4:
            assert len({tuple(r) for r in s[:5]}) > 1, "the permutation differs from row to row"
        # the float64 two-pass statistics of the definition give the stated values, whatever the order (here numpy's)
        mu, rstd, dev = TD.N.ln_stats(z, TD.NORM_EXACT_EPS)
        assert np.all(mu == base) and np.all(rstd == 0.5) and np.all(np.abs(dev) == 1.0)
        for act in TD.EXACT_ACTS:
            stats, out, dgamma, dbeta, share = TD.norm_exact_model(rows, cols, base, act)
            ref = TD.N.ln_backward(g, z, gamma, beta, TD.NORM_EXACT_EPS, act, np.longdouble)
            fwd = TD.N.ln_forward(z, gamma, beta, TD.NORM_EXACT_EPS, act, np.longdouble)[0]
            assert np.array_equal(out.astype(np.longdouble), fwd) and np.array_equal(dgamma.astype(np.longdouble), ref[1])
            assert np.array_equal(dbeta.astype(np.longdouble), ref[2]) and not np.any(np.signbit(out) & (out == 0))
            assert (share == 1.0) if act == "identity" else (0.3 < share < 0.7 if cols > 100 else 0.0 < share < 1.0), "relu gates a good part of the entries"
            assert np.count_nonzero(dgamma) >= 0.5 * cols and np.count_nonzero(dbeta) >= 0.5 * cols


# ------------------------------------------------------------------------------------------------ the column sums
def test_colsum_table_and_caps():
    assert {TD.colsum_width(*c) for c in TD.COLSUM_CASES} == {1, 2}
    for w, tile in ((1, 32), (2, 64)):  # both sides of a column tile of 32 lanes x W
        widths = {c for c, m in TD.COLSUM_CASES if TD.colsum_width(c, m) == w}
        assert {tile - 1 if w == 1 else tile - 2, tile, tile + 1 if w == 1 else tile + 2} <= widths | {62}
        assert any(c < tile for c in widths) and any(c > 2 * tile for c in widths)
    assert 62 not in TD.COLSUM_COLS and {63, 64, 65, 66} <= set(TD.COLSUM_COLS), "64 / 66 are the two sides at W = 2, 63 / 65 run W = 1"
    assert all(TD.colsum_plan(r) == (1, r) for r in TD.COLSUM_ROWS if r <= 256) and TD.colsum_plan(257) == (2, 129) and TD.colsum_plan(513) == (3, 171)
    assert {r % 8 for r in TD.COLSUM_ROWS} >= {0, 1, 7}, "the eight row phases: full, one over, one short"
    assert TD.colsum_plan(150001) == (512, 293) and TD.colsum_plan(131072) == (512, 256) and TD.colsum_plan(131073) == (511, 257)
    for rows, cols, capped in TD.COLSUM_CAPS:
        assert (-(-rows // 256) > TD.COLSUM_RANGES) == capped
        TD.colsum_data(rows, cols)
    hip = K.load()
    for rows in TD.COLSUM_ROWS + [150001, 131072, 131073, 5000]:
        assert hip.hnh_colsum_f64_workspace(rows, 6) == TD.colsum_plan(rows)[0] * 6, rows


# ------------------------------------------------------------------------------------------------ the gradient kernels
def test_grad_table_reaches_every_lane_group():
    assert set(TD.ISSUE_GRAD_WIDTHS) < set(TD.GRAD_WIDTHS)
    groups = {c: TD.lane_group(c[0], TD.grad_vec(*c)) for c in TD.GRAD_CASES}
    assert set(groups.values()) == {(w, l) for w in (1, 2) for l in range(7)}
    # what the width lists {1, 3, 7, 64, 100, 256} never ran
    for f, g in ((2, (2, 0)), (4, (2, 1)), (8, (2, 2)), (16, (2, 3)), (32, (2, 4))):
        assert groups[(f, True)] == g
    for f, g in ((2, (1, 1)), (16, (1, 4)), (17, (1, 5)), (32, (1, 5))):
        assert groups[(f, False)] == g
    assert groups[(130, True)] == (2, 6) and groups[(65, False)] == (1, 6) and 130 > 2 * 64, "the trip loop takes a second, ragged trip"
    for c in TD.GRAD_CASES:
        lay = TD.grad_layout(*c)
        par = {v % 2 for k, v in lay.items() if k != "col0"}
        assert par == ({0} if c[1] else {1}) and (not c[1] or lay["col0"] % 2 == 0)
        g = 256 >> groups[c][1]
        assert TD.grad_rows(*c) == [g - 1, g, g + 1]


def test_past_cap_sizes():
    (r17, c17, ld17, col17), (r34, c34, ld34, col34), (_, _, _, odd34) = TD.ADDEND_PAST
    assert r17 * c17 == D.PAST_PLAIN == r34 * (c34 // 2) and D.ew_trips(r17 * c17, TD.EW_CAP) == 3 and D.PAST_PLAIN % TD.EW_CAP == 259
    assert list(TD.ADDEND_PAST.values()) == [1, 2, 1] and col34 % 2 == 0 and odd34 % 2 == 1 and ld34 % 2 == 0 and D.ew_trips(r34 * c34, TD.EW_CAP) == 5
    assert all(col0 + cols <= ld for _, cols, ld, col0 in TD.ADDEND_PAST)
    # the optimizer: a full trip of 1024 workgroups and 1281 elements more; 262 144 elements fill the grid exactly
    rows, cols, pitch = TD.OPTIM_BIG
    assert rows * cols == 263425 and TD.optim_blocks(rows * cols) == (1024, 2) and rows * cols - 1024 * 256 == 1281 and pitch == cols + 2
    assert TD.optim_blocks(262144) == (1024, 1) and TD.optim_blocks(262145) == (1024, 2) and TD.optim_blocks(257) == (2, 1)
    first = TD.OPTIM_TABLE[:K.OPTIM_MAX_TENSORS]
    assert K.OPTIM_MAX_TENSORS < len(TD.OPTIM_TABLE) and (rows, cols, 2) in first
    assert {r * c for r, c, _ in first} >= {1, 255, 256, 257, 262144} and max(r * c for r, c, _ in TD.OPTIM_TABLE[K.OPTIM_MAX_TENSORS:]) < 1024 * 256
    assert TD.CLIP_QUARTER_MAX_NORM / (np.sqrt(sum(TD.CLIP_QUARTER_SUMS)) + 1e-6) == 0.25, "the coefficient of the clipped SGD steps is exactly 0.25"
    # the sum of squares
    units = {n: TD.sumsq_units(*s[:3]) for n, s in TD.SUMSQ_BIG.items()}
    assert units["dense"] == (2, 4195538, 4195538) and 2 * 4195538 == 8391076 and TD.sumsq_blocks(4195538) == (2048, 9)
    assert TD.sumsq_blocks(4194304) == (2048, 8) and TD.sumsq_blocks(300001) == (147, 8), "the cap's last size, and the largest earlier tensor"
    assert units["pitched"] == (1, 3, 4200003) and TD.sumsq_blocks(4200003) == (2048, 9) and 2048 * 256 // 3 == 174762
    assert units["long_rows"] == (1, 700001, 2100003) and TD.sumsq_blocks(2100003) == (1026, 8) and 1026 * 256 < 700001
    assert max(r * p for r, c, p, _ in TD.SUMSQ_BIG.values()) * 8 < 70e6, "the largest allocation"


# ------------------------------------------------------------------------------------------------ on the second test double
@pytest.fixture(scope="module")
def double():
    lib = DC.bind(T.ORACLE_GAT_BACKEND)
    assert lib.hnh_backend_name() == b"oracle-cpu-test-double-gat"
    lib.hnh_oracle_order_report.restype = C.c_long
    lib.hnh_oracle_order_accesses.restype = C.c_long
    lib.hnh_oracle_order_enable(1)
    ctx = DC.Api(lib)
    yield lib, ctx
    ctx.close()


def drain(lib):
    buf = C.create_string_buffer(16384)
    return lib.hnh_oracle_order_report(buf, 16384), buf.value.decode()


def watched(lib, fn):
    assert drain(lib) == (0, ""), "reports left behind by an earlier test"
    before = lib.hnh_oracle_order_accesses()
    out = fn()
    assert drain(lib) == (0, ""), "no race and no MISUSE"
    assert lib.hnh_oracle_order_accesses() > before, "the case was watched"
    return out


@pytest.mark.parametrize("case", TD.GRAD_CASES, ids=[TD.grad_id(c) for c in TD.GRAD_CASES])
def test_act_grad_cols_on_the_double(double, case):
    lib, ctx = double
    for rows in TD.grad_rows(*case):
        dz, delta = watched(lib, lambda: TD.act_grad(ctx, rows, *case))
        assert np.count_nonzero(dz) >= 0.3 * dz.size and (case[0] < 4 or np.count_nonzero(delta) >= 0.5 * rows), "results that cannot pass for the fill"


def test_exact_sgd_past_the_cap_on_the_double(double):
    lib, ctx = double
    watched(lib, lambda: TD.optim_exact_sgd(ctx, "plain"))


def test_adam_past_the_cap_on_the_double(double):
    lib, ctx = double
    assert watched(lib, lambda: TD.optim_adam(ctx)) <= T.TOL


def test_exactness_checks_are_checked():
    TD.exact_sum(np.array([2.0 ** 53 - 1, 0.0]))
    for bad in (np.array([2.0 ** 53]), np.array([0.5])):
        with pytest.raises(AssertionError):
            TD.exact_sum(bad)
    TD.exact_sum(np.array([0.5]), unit=0.5)
    TD.dyadic(np.array([2.0 ** -20, 1000.5]))
    for bad in (np.array([2.0 ** -21]), np.array([2.0 ** 20]), np.array([1.0 / 3.0])):
        with pytest.raises(AssertionError):
            TD.dyadic(bad)
