"""The design of tests/gram_cases.py without a GPU (hnh_gram_rows_f64 is in neither CPU test double: tests/test_gram_instances_gpu.py runs
the kernel).

The table: all ten (instance, load width) pairs, every listed width and every row class per instance, X and every other operand moved
by 8 bytes per instance, at most 70 cases, none larger than 593 x 256.
The exact cg design, on the model alone: the int64 model's exactness assertions and the live share at EVERY case; at one case per
instance a float64 evaluation with every sum forward and with every sum reversed equals the model in x, r and rs bit for bit, while p
from a separate multiply and add differs from the once-rounded p somewhere (the share is printed: 9 .. 13 % of the entries), so the
device's p is compared sharply; the planted rows behave as listed.
The operator additions in composed mode on the second CPU test double under the stream-order checker, and the float64 definition against
long double at their widths and inputs within T.TOL / 10 (the rule of tests/test_als_implicit_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import als_common
import als_implicit_common as IC
import als_implicit_ref as IR
import gram_cases as G
import hnh_testlib as T
from distributed_sddmm_amd import api as H
from row_pass_cases import same_bits

TOPS = sorted(G.INSTANCES)


@pytest.fixture
def gat_double():
    """the second CPU test double with the stream-order checker on, as in tests/test_als_implicit_cpu.py"""
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


def of_instance(top):
    return [c for c in G.CASES if G.instance_of(c[1], True)[:3] == G.INSTANCES[top]]


def model_cases():
    """one case per instance: the fewest rows with at least 20"""
    return [min((c for c in of_instance(top) if c[0] >= 20), key=lambda c: (c[0], c[1])) for top in TOPS]


# ------------------------------------------------------------------------------------------------ the table
def test_instance_of_restates_the_header():
    want = {1: (1, 2, 8), 16: (1, 2, 8), 17: (2, 2, 8), 32: (2, 2, 8), 33: (4, 2, 8), 64: (4, 2, 8), 65: (8, 1, 8), 128: (8, 1, 8), 129: (16, 1, 4),
            256: (16, 1, 4)}
    for R, inst in want.items():
        for aligned in (True, False):
            assert G.instance_of(R, aligned) == inst + (R % 4 == 0 and aligned,)
    assert [G.tile_rows(t) for t in TOPS] == [(32, 256), (32, 256), (32, 256), (16, 128), (16, 64)]
    header = open(T.ROOT + "/include/hnh_als_implicit.h").read()
    assert "#define HNH_GRAM_MAX_R 256" in header and max(TOPS) == 256


def test_the_table_reaches_every_instance_with_both_load_widths():
    pairs = {G.instance_of(R, xs == 0) for rows, R, xs, _ in G.CASES if rows > 0}
    assert pairs == {inst + (vec,) for inst in G.INSTANCES.values() for vec in (True, False)} and len(pairs) == 10
    older = {G.instance_of(R, True) for R in (2, 8, 17, 100, 128, 130, 256)}  # test_als_implicit_gpu.py's widths, every buffer aligned
    never_ran = sorted(pairs - older)
    print("(instance, 16-byte loads) pairs the older tests never launched:", never_ran)
    assert never_ran == [(2, 2, 8, True), (4, 2, 8, False), (4, 2, 8, True), (8, 1, 8, False)]


@pytest.mark.parametrize("top", TOPS)
def test_the_table_has_every_width_and_row_class(top):
    cases = of_instance(top)
    wd = G.WIDTHS[top]
    have = {(R, xs) for _, R, xs, _ in cases}
    assert (top, 0) in have and (top, 8) in have, "the exact top width with 16-byte loads, and with X moved by 8 bytes"
    for R in (wd["first"], wd["odd"]) + wd["partial"]:
        assert any(r == R for r, _ in have), R
    assert wd["first"] == {16: 1, 32: 17, 64: 33, 128: 65, 256: 129}[top] and wd["odd"] == top - 1
    assert wd["partial"][0] == {16: 4, 32: 20, 64: 48, 128: 100, 256: 252}[top]
    assert any(R % 4 == 0 and R % 16 != 0 and xs == 0 for R, xs in have), "16-byte loads meet k + 4 <= R on both sides in the last K tile"
    t, w = G.tile_rows(top)
    assert G.row_counts(top) == [0, 1, t - 1, t, t + 1, w - 1, w, w + 1, 2 * w + t + 1]
    assert set(G.row_counts(top)) <= {c[0] for c in cases}
    assert any(c[3] == 8 for c in cases) and any(c[3] == 0 for c in cases), "Out, G, x, r, rs moved by 8 bytes in a case of every instance"
    assert any(c[0] > w and G.instance_of(c[1], c[2] == 0)[3] for c in cases) and any(c[0] > w and c[1] % 4 == 0 and c[2] == 8 for c in cases)
    assert any(c[0] >= 8 and c[3] == 8 for c in cases), "... in a case with planted rows"


def test_the_table_is_a_small_covering_subset():
    assert len(G.CASES) == len(set(G.CASES)) == 66 <= 70
    assert max(G.CASES, key=lambda c: c[0] * c[1])[:2] == G.MOST == (593, 256) and max(c[0] for c in G.CASES) == 593
    for rows, R, xs, os_ in G.CASES:
        assert 0 <= rows and 1 <= R <= 256 and xs in (0, 8) and os_ in (0, 8)
    assert sum(G.expected_launches().values()) == 4 * sum(1 for c in G.CASES if c[0]) and min(G.expected_launches().values()) > 0
    for rows in (8, 9, 31, 593):
        at = G.planted_rows(rows)
        assert sorted(at) == sorted(G.PLANTED) and at["frozen"] == 1 and at["exact"] == rows - 1
    assert G.planted_rows(7) == {}


# ------------------------------------------------------------------------------------------------ the exact cg design
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_the_model_is_exact_and_its_rows_are_live(case):
    """cg_model() asserts that every exact quantity is a multiple of its scale below 2^53; without cg the sums are bounded likewise"""
    rows, R = case[:2]
    G.plain_operands(case)
    want, ops = G.cg_model(case), G.cg_operands(case)
    assert want["bits"] <= 52
    if case[:2] == G.MOST:
        print("the widest exact quantity of the largest case: %d bits" % want["bits"])
    share = G.live_share(case)
    if rows >= 20:
        assert share >= 0.9, share
    assert share == 1.0 or rows == 0, "with G = Y^T Y + 64 I every row that is not planted is live"
    plant = G.planted_rows(rows)
    assert bool(plant) == (rows >= 8)
    if plant:
        assert not want["live"][[plant[k] for k in G.PLANTED[:4]]].any() and want["live"][plant["exact"]]
        assert ops["rs"][plant["frozen"]] == 0 and ops["rs"][plant["negrs"]] < 0 and not ops["p"][plant["pzero"]].any() and ops["rs"][plant["pzero"]] > 0
        mp = ops["out"] + ops["p"] @ ops["g"]
        assert IR.rowdot(ops["p"], mp)[plant["uphill"]] < 0 and ops["rs"][plant["uphill"]] > 0
        assert IR.rowdot(ops["p"], mp)[plant["pzero"]] == 0
        G.check_planted(case, ops, want, "model")
        assert want["beta"][plant["exact"]] == 0.0
        for k in G.PLANTED[:4]:
            assert np.signbit(ops["x"][plant[k], 0]) and np.signbit(ops["r"][plant[k], R - 1]), "the -0.0 a recomputed row would lose"


@pytest.mark.parametrize("case", model_cases(), ids=G.case_id)
def test_every_order_of_addition_gives_the_model_and_unfused_p_does_not(case):
    want = G.cg_model(case)
    live = want["live"]
    for reverse in (False, True):
        got = G.float_eval(case, reverse)
        assert np.array_equal(got["live"], live)
        for k in ("x", "r", "rs"):
            assert np.array_equal(got[k], want[k]), (k, reverse)
    unfused = G.float_eval(case, False)["p"]
    differ = int((unfused[live] != want["p"][live]).sum())
    print("gram cg %s: p from a separate multiply and add differs from the once-rounded p in %d of %d entries (%.1f %%)"
          % (G.case_id(case), differ, want["p"][live].size, 100.0 * differ / want["p"][live].size))
    assert differ > 0, "the comparison of p must tell an fma from a multiply and an add"
    assert np.array_equal(unfused[~live], want["p"][~live])
    assert float(np.abs(unfused - want["p"]).max()) <= 2.0 ** -40 * float(np.abs(want["p"]).max()), "... and no more than a rounding apart"


def test_model_cases_are_one_per_instance():
    cases = model_cases()
    assert [G.instance_of(c[1], True)[:3] for c in cases] == [G.INSTANCES[t] for t in TOPS]
    assert all(20 <= c[0] <= 127 for c in cases)


# ------------------------------------------------------------------------------------------------ the operator, composed, on the double
def watched(gat_double, run):
    assert drain(gat_double) == (0, ""), "reports left behind by an earlier test"
    before = gat_double.hnh_oracle_order_accesses()
    out = run()
    assert drain(gat_double) == (0, ""), "no race and no MISUSE"
    assert gat_double.hnh_oracle_order_accesses() > before, "the case was watched"
    return out


@pytest.mark.parametrize("case", G.OPERATOR_WIDTHS, ids=als_common.case_id)
def test_composed_mode_at_the_new_widths(gat_double, case):
    worst, _ = watched(gat_double, lambda: G.run_widths(case, "cpu"))
    print("gram widths %s composed on the double: %.2e" % (case, worst))
    assert worst <= T.TOL


def test_composed_mode_keeps_rows_that_are_not_live_at_zero(gat_double):
    worst = watched(gat_double, lambda: G.run_dead_rows(False))
    print("gram dead rows composed on the double: %.2e" % worst)
    assert worst <= T.TOL


def test_composed_mode_with_zero_weights(gat_double):
    worst = watched(gat_double, lambda: G.run_zero_weights(False))
    print("gram zero weights composed on the double: %.2e" % worst)
    assert worst <= T.TOL


def test_the_operator_cases_are_the_ones_listed():
    assert G.OPERATOR_WIDTHS == [("hub", 16, 1, 1), ("hub", 16, 4, 1), ("hub", 32, 1, 1), ("hub", 32, 4, 1), ("hub", 64, 1, 1), ("hub", 64, 4, 1),
                                 ("hub", 48, 4, 2)]
    for g, R, p, c in G.OPERATOR_WIDTHS + [("hub", G.DEAD_R, G.DEAD_P, 1), G.ZERO_W]:
        assert T.valid_config(IC.ALG, p, c, R)
    case, _ = G.dead_rows_case()
    assert case["M"] % G.DEAD_P and case["N"] % G.DEAD_P, "every rank has padding rows"
    assert (IC.STEPS, IC.ITERS) == (2, 2)


def protocol_error(case, want):
    a, b, losses = IR.run(case["rows"], case["cols"], case["w"], case["A"], case["B"], IR.LAMBDA, IC.STEPS, IC.ITERS, np.longdouble)
    return float(max(T.rel(want["A"], a), T.rel(want["B"], b), T.rel(want["losses"], losses)))


@pytest.mark.parametrize("R", [16, 32, 48, 64])
def test_float64_is_a_good_enough_model_at_the_new_widths(R):
    err = protocol_error(IR.inputs("hub", R), IR.expected("hub", R))
    print("observed float64 against long double at R = %d, the operator tests' protocol: %.2e" % (R, err))
    assert err <= T.TOL / 10


@pytest.mark.parametrize("which", ["dead_rows", "zero_weights"])
def test_float64_is_a_good_enough_model_of_the_varied_inputs(which):
    case, want = G.dead_rows_case() if which == "dead_rows" else G.zero_weight_case()
    err = protocol_error(case, want)
    print("observed float64 against long double, %s: %.2e" % (case["name"], err))
    assert err <= T.TOL / 10
    assert same_bits(want["A"], G._expected(case)["A"])
