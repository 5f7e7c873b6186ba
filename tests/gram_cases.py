"""What tests/test_gram_instances_cpu.py and tests/test_gram_instances_gpu.py share (not itself a test): the case table of
hnh_gram_rows_f64 (include/hnh_als_implicit.h), the exact operands of both of its modes with their host models, the guarded calls, and
the operator cases of api.ImplicitALS at the widths and rows the older files do not reach.  On the pattern of tests/dense_cases.py;
Guarded, same_bits and describe are tests/row_pass_cases.py's.

THE TABLE.  The dispatcher picks gram_rows_kernel<NJ, MI, WAVES> by R (<1,2,8> R <= 16, <2,2,8> R <= 32, <4,2,8> R <= 64, <8,1,8>
R <= 128, <16,1,4> R <= 256) and loads X with 16-byte loads when R % 4 == 0 and X is 16-byte aligned, else with 8-byte loads:
instance_of() restates that from the header.  A wave owns T = 16 MI rows, a workgroup W = WAVES T.  Per instance the table has the
widths WIDTHS (the top width aligned and with X moved by 8 bytes, the first width, an odd width below the top, widths of R % 4 == 0
whose last K tile of 16 is partial) and the row counts 0, 1, T - 1, T, T + 1, W - 1, W, W + 1, 2 W + T + 1, as a covering subset: 13
cases per instance, and one case of 593 x 256 (nine workgroups of <16,1,4>, a wave tile and one row; the widest row at the most rows).
A case is (rows, R, x_shift, others_shift): the bytes by which X (= p in cg mode) and by which Out, G, x, r, rs and rowdot are moved
off their 128-byte alignment (0 or 8).  R = 48 is listed among the "partial" widths by the issue that asked for this table although
48 = 3 x 16; it stays, and 52 beside it is the width of that instance whose last K tile is partial.

WITHOUT cg.  Out, X, G are integers of [-4, 4]: Mp = Out + X G and rowdot = <X, Mp> are exact in every order of addition.

WITH cg.  Out, p, r, x are integers of [-4, 4]; G = Y^T Y + 64 I with a 3 x R integer Y of [-2, 2] (integer, symmetric, <p, Mp> >= 60
|p|^2 > 0 for p != 0); alpha is drawn per row from ALPHAS (multiples of 2^-6) and the INPUT rs = alpha <p, Mp> is formed on the host.
Then Mp, bdot, rs / bdot = alpha (a correctly rounded quotient of an exact ratio), x + alpha p, r - alpha Mp and rsnew = <r, r> are
multiples of 2^-12 below 2^53 2^-12 in every order of addition, fused or not: cg_model() evaluates them in int64 scaled by 64 and 4096
and asserts those bounds.  beta = rsnew / rs is ONE correctly rounded division (the library is built without fast-math) and p =
fma(beta, p, r) ONE rounding: the model takes beta from a float64 division and p from fractions.Fraction, rounded once by float().
Five rows are planted where rows >= 8 (planted_rows()): rs == 0; bdot < 0 (Out = -p G - p); p == 0 with rs > 0 (bdot == 0); rs < 0 —
x and r keep their bytes (each holds a -0.0, which x + 0 p would lose), p gets r's bytes, rs = <r, r>; and a LIVE row with r = alpha Mp:
rsnew == 0, beta == 0, the new p is zero.  Every other row is live in the model (live_share()).

Every comparison is an equality of bit patterns but that of the -0.0-free live rows' values, which numpy's array_equal compares as
numbers; the operator cases are held to T.TOL like tests/test_als_implicit_gpu.py's."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np

import als_implicit_common as IC
import als_implicit_ref as IR
import hnh_testlib as T
import row_pass_cases as RC
from distributed_sddmm_amd import _kernels as K
from row_pass_cases import Guarded, same_bits

INVALID = 1
SENTINEL = -7.25e77   # rowdot's fill: a finite value no result takes
# top width -> (NJ, MI, WAVES), as the header and DESIGN 6c list them
INSTANCES = {16: (1, 2, 8), 32: (2, 2, 8), 64: (4, 2, 8), 128: (8, 1, 8), 256: (16, 1, 4)}
# per instance: first width, odd width below the top, widths of R % 4 == 0 with a partial last K tile (and the issue's 48)
WIDTHS = {16: dict(first=1, odd=15, partial=(4,)), 32: dict(first=17, odd=31, partial=(20,)), 64: dict(first=33, odd=63, partial=(48, 52)),
          128: dict(first=65, odd=127, partial=(100,)), 256: dict(first=129, odd=255, partial=(252,))}
ALPHAS = np.array([1.0, 0.5, 0.25, 0.375, 2.0 ** -6, 3 * 2.0 ** -5])
PLANTED = ("frozen", "uphill", "pzero", "negrs", "exact")
MOST = (593, 256)


def instance_of(R, x_aligned):
    """(NJ, MI, WAVES, vec) of the launch hnh_gram_rows_f64 makes at width R; x_aligned = X is 16-byte aligned"""
    assert 1 <= R <= 256
    top = min(t for t in INSTANCES if R <= t)
    return INSTANCES[top] + (R % 4 == 0 and bool(x_aligned),)


def tile_rows(R):
    """(T, W): the rows of a wave and of a workgroup at width R"""
    _, mi, waves, _ = instance_of(R, True)
    return 16 * mi, 16 * mi * waves


def row_counts(top):
    t, w = tile_rows(top)
    return [0, 1, t - 1, t, t + 1, w - 1, w, w + 1, 2 * w + t + 1]


def _table():
    cases = []
    for top, wd in WIDTHS.items():
        rows = row_counts(top)
        configs = [(top, 0), (top, 8), (wd["first"], 0), (wd["odd"], 0), (wd["partial"][0], 0)]
        for i, n in enumerate(rows):                       # every row count once, the five width configurations in turn
            R, xs = configs[i % 5]
            cases.append((n, R, xs, 8 if i in (1, 4, 8) else 0))
        big, w1 = rows[-1], rows[-2]
        cases += [(big, top, 0, 0), (big, top, 8, 8), (big, wd["partial"][-1], 0, 8), (w1, wd["odd"], 8, 0)]
    cases.append(MOST + (0, 0))
    return cases


CASES = _table()


def case_id(c):
    return "%dx%d_x%d_o%d" % c


def expected_launches():
    """(NJ, MI, WAVES) -> launches of one run of tests/test_gram_instances_gpu.py: a case with rows > 0 launches four times (rowdot given
    and NULL, cg twice); the refusals and rows == 0 launch nothing"""
    out = {inst: 0 for inst in INSTANCES.values()}
    for rows, R, xs, _ in CASES:
        if rows:
            out[instance_of(R, xs == 0)[:3]] += 4
    return out


def _seed(case):
    rows, R, xs, os_ = case
    return ((rows * 257 + R) * 2 + xs // 8) * 2 + os_ // 8


def ints(rng, k, shape):
    return rng.integers(-k, k + 1, shape).astype(np.float64)


# ------------------------------------------------------------------------------------------------ without cg
@functools.lru_cache(maxsize=None)
def plain_operands(case):
    rows, R = case[:2]
    rng = np.random.default_rng(_seed(case))
    out, x, g = ints(rng, 4, (rows, R)), ints(rng, 4, (rows, R)), ints(rng, 4, (R, R))
    mp = out + x @ g
    ops = dict(out=out, x=x, g=g, mp=mp, rowdot=IR.rowdot(x, mp))
    assert np.abs(out).sum(initial=0) + (np.abs(x) @ np.abs(g)).max(initial=0) * R * 4 < 2.0 ** 53
    for a in ops.values():
        a.setflags(write=False)
    return ops


class Buffers:
    """The guarded device arrays of one call: `moved` names those 8 bytes off their alignment.  fetch(): every array, its guards asserted."""

    def __init__(self, ctx, arrays, moved=()):
        self.ctx = ctx
        self.a = {k: Guarded(ctx, np.ascontiguousarray(v, dtype=np.float64), int(k in moved), k) for k, v in arrays.items()}
        for k, g in self.a.items():
            assert g.ptr % 16 == (8 if k in moved else 0)

    def ptr(self, name):
        return self.a[name].ptr

    def fetch(self, what):
        self.ctx.sync()
        got = {}
        for k, g in self.a.items():
            got[k], guards = g.fetch()
            assert guards, "%s: a guard of %s was overwritten" % (what, k)
        return got

    def free(self):
        for g in self.a.values():
            g.free()


def call(ctx, out, x, g, rows, R, rowdot=None, cg=None):
    return ctx.lib.hnh_gram_rows_f64(ctx.h, out, x, g, rows, R, rowdot, C.byref(cg) if cg is not None else None, K.STREAM_COMPUTE)


def moved_names(case, x_name):
    return ({x_name} if case[2] else set()) | ({"out", "g", "x", "r", "rs", "dot"} - {x_name} if case[3] else set())


def run_plain(ctx, case):
    """cg == NULL, rowdot given and NULL: Out and rowdot are the model's bits, X and G come back, rowdot beyond `rows` is untouched"""
    rows, R = case[:2]
    ops = plain_operands(case)
    dot0 = np.full(rows + 3, SENTINEL)
    for with_dot in (True, False):
        what = "%s %s" % (case_id(case), "rowdot" if with_dot else "no rowdot")
        b = Buffers(ctx, dict(out=ops["out"], x=ops["x"], g=ops["g"], dot=dot0), moved_names(case, "x"))
        ctx.check(call(ctx, b.ptr("out"), b.ptr("x"), b.ptr("g"), rows, R, b.ptr("dot") if with_dot else None), what)
        got = b.fetch(what)
        b.free()
        assert np.array_equal(got["out"], ops["mp"]), "%s: Out: %s" % (what, RC.describe(got["out"], ops["mp"]))
        assert same_bits(got["x"], ops["x"]) and same_bits(got["g"], ops["g"]), "%s: X and G are read only" % what
        want_dot = np.concatenate([ops["rowdot"], dot0[rows:]]) if with_dot else dot0
        assert np.array_equal(got["dot"], want_dot), "%s: rowdot: %s" % (what, RC.describe(got["dot"], want_dot))


# ------------------------------------------------------------------------------------------------ with cg
def planted_rows(rows):
    """kind -> row, for rows >= 8: spread from the second row to the last one, so that the first and the last wave tile hold one"""
    if rows < 8:
        return {}
    at = np.linspace(1, rows - 1, len(PLANTED)).astype(int)
    assert len(set(at.tolist())) == len(PLANTED)
    return dict(zip(PLANTED, at.tolist()))


@functools.lru_cache(maxsize=None)
def cg_operands(case):
    """dict(out, g, x, r, p, rs, alpha) of the case, planted rows included"""
    rows, R = case[:2]
    rng = np.random.default_rng(_seed(case) + 1_000_003)
    out, x, r, p = (ints(rng, 4, (rows, R)) for _ in range(4))
    p[~np.any(p != 0, axis=1), 0] = 1.0                       # every row has a direction (R = 1 draws p == 0 one time in nine)
    y = ints(rng, 2, (3, R))
    g = y.T @ y + 64.0 * np.eye(R)
    alpha = rng.choice(ALPHAS, rows)
    plant = planted_rows(rows)
    if plant:
        p[plant["pzero"]] = 0.0
        out[plant["uphill"]] = -(p[plant["uphill"]] @ g) - p[plant["uphill"]]
    mp = out + p @ g
    rs = alpha * IR.rowdot(p, mp)
    if plant:
        rs[plant["frozen"]], rs[plant["uphill"]], rs[plant["pzero"]] = 0.0, 3.0, 2.0
        rs[plant["negrs"]] = -rs[plant["negrs"]]
        r[plant["exact"]] = alpha[plant["exact"]] * mp[plant["exact"]]
        for kind in ("frozen", "uphill", "pzero", "negrs"):   # a -0.0 each: lost by x + 0 p and by r - 0 Mp, kept by "not stored"
            x[plant[kind], 0], r[plant[kind], R - 1] = -0.0, -0.0
    ops = dict(out=out, g=g, x=x, r=r, p=p, rs=rs, alpha=alpha)
    for a in ops.values():
        a.setflags(write=False)
    return ops


def _exact_int(a, scale):
    """a * scale as int64, asserted to be whole and below 2^53"""
    s = a * scale
    i = np.rint(s).astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s) and np.abs(i).max(initial=0) < 2 ** 53, "an operand is not a multiple of 1 / %d" % scale
    return i


@functools.lru_cache(maxsize=None)
def cg_model(case):
    """dict(x, r, p, rs, live) after the guarded update, and `bits`: the widest exact quantity in bits.  Exact quantities in int64 (x and r
    scaled by 64, sums of squares by 4096), each asserted below 2^53 by the sum of its terms' absolute values, which bounds every
    partial sum in every order; beta by one float64 division; p by exact rational arithmetic rounded once."""
    rows, R = case[:2]
    o = cg_operands(case)
    out, g, p = (_exact_int(o[k], 1) for k in ("out", "g", "p"))
    x64, r64, a64 = _exact_int(o["x"], 64), _exact_int(o["r"], 64), _exact_int(o["alpha"], 64)
    rs_in = o["rs"]
    widest = 0

    def bounded(abs_sum):
        nonlocal widest
        m = int(abs_sum.max(initial=0))
        assert m < 2 ** 53, "a sum leaves the exactly representable range"
        widest = max(widest, m.bit_length())

    bounded(np.abs(out) + np.abs(p) @ np.abs(g))
    mp = out + p @ g
    bounded((np.abs(p) * np.abs(mp)).sum(axis=1))
    bdot = (p * mp).sum(axis=1)
    live = (rs_in > 0) & (bdot > 0)
    # the input rs is alpha bdot exactly, so the device's correctly rounded rs / bdot is alpha itself
    plant = planted_rows(rows)
    made = np.ones(rows, dtype=bool)
    for kind in ("frozen", "uphill", "pzero", "negrs"):
        if plant:
            made[plant[kind]] = False
    assert np.array_equal(_exact_int(rs_in[made], 64), (a64 * bdot)[made]) and np.array_equal((rs_in / np.where(live, bdot, 1))[live], o["alpha"][live])
    a = np.where(live, a64, 0)[:, None]
    bounded(np.abs(x64) + np.abs(a * p))
    bounded(np.abs(r64) + np.abs(a * mp))
    xn64, rn64 = x64 + a * p, r64 - a * mp
    bounded((rn64 * rn64).sum(axis=1))
    rsn4096 = (rn64 * rn64).sum(axis=1)
    xn, rn, rsn = xn64 / 64.0, rn64 / 64.0, rsn4096 / 4096.0
    xn[~live], rn[~live] = o["x"][~live], o["r"][~live]      # the bytes, a -0.0 included
    beta = np.where(live, rsn / np.where(live, rs_in, 1.0), 0.0)
    pn = rn.copy()
    for i in np.nonzero(live)[0].tolist():
        n, d = float(beta[i]).as_integer_ratio()
        b = Fraction(n, d)
        pn[i] = [float(b * pj + Fraction(rj, 64)) for pj, rj in zip(p[i].tolist(), rn64[i].tolist())]
    res = dict(x=xn, r=rn, p=pn, rs=rsn, live=live, beta=beta, bits=widest)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def live_share(case):
    """the share of live rows among those that are not planted not-live, in the model"""
    rows = case[0]
    plant = planted_rows(rows)
    dead = {plant[k] for k in PLANTED[:4]} if plant else set()
    keep = np.array([i not in dead for i in range(rows)], dtype=bool)
    return float(cg_model(case)["live"][keep].mean()) if keep.any() else 1.0


def check_planted(case, ops, res, what):
    plant = planted_rows(case[0])
    for kind in PLANTED[:4] if plant else ():
        k = plant[kind]
        assert same_bits(res["x"][k], ops["x"][k]) and same_bits(res["r"][k], ops["r"][k]), "%s: the %s row keeps the bytes of x and r" % (what, kind)
        assert same_bits(res["p"][k], ops["r"][k]), "%s: the %s row gets p = r, bit for bit" % (what, kind)
        assert res["rs"][k] == IR.rowdot(ops["r"][k:k + 1], ops["r"][k:k + 1])[0]
    if plant:
        k = plant["exact"]
        assert res["rs"][k] == 0.0 and np.all(res["p"][k] == 0.0) and np.all(res["r"][k] == 0.0), "%s: the row with r = alpha Mp" % what


def float_eval(case, reverse, fused_p=False):
    """The update in plain float64, every sum in the given order of k (forward or reversed), multiplies and adds separate; p unfused"""
    o = cg_operands(case)
    rows, R = case[:2]
    order = list(range(R))[::-1] if reverse else list(range(R))
    mp = np.zeros((rows, R))
    for k in order:
        mp = mp + o["p"][:, k:k + 1] * o["g"][k]
    mp = mp + o["out"]

    def dot(a, b):
        s = np.zeros(rows)
        for k in order:
            s = s + a[:, k] * b[:, k]
        return s

    bdot = dot(o["p"], mp)
    live = (o["rs"] > 0) & (bdot > 0)
    alpha = np.where(live, o["rs"] / np.where(live, bdot, 1), 0)
    xn = np.where(live[:, None], o["x"] + alpha[:, None] * o["p"], o["x"])
    rn = np.where(live[:, None], o["r"] - alpha[:, None] * mp, o["r"])
    rsn = dot(rn, rn)
    beta = np.where(live, rsn / np.where(live, o["rs"], 1), 0)
    return dict(x=xn, r=rn, rs=rsn, p=np.where(live[:, None], rn + beta[:, None] * o["p"], rn), live=live)


def run_cg(ctx, case):
    """cg given, twice: x, r, p, rs are the model's; Out, G and rowdot come back untouched; the guards hold; two runs give the same bytes"""
    rows, R = case[:2]
    ops, want = cg_operands(case), cg_model(case)
    if rows >= 20:
        assert live_share(case) >= 0.9, "the model's rows must be live"
    dot0 = np.full(rows + 3, SENTINEL)
    runs = []
    for trip in range(2):
        what = "%s cg run %d" % (case_id(case), trip)
        b = Buffers(ctx, dict(out=ops["out"], g=ops["g"], x=ops["x"], r=ops["r"], p=ops["p"], rs=ops["rs"], dot=dot0), moved_names(case, "p"))
        cg = K.GramCg(b.ptr("x"), b.ptr("r"), b.ptr("p"), b.ptr("rs"))
        ctx.check(call(ctx, b.ptr("out"), b.ptr("p"), b.ptr("g"), rows, R, b.ptr("dot"), cg), what)
        runs.append(b.fetch(what))
        b.free()
    got = runs[0]
    what = case_id(case) + " cg"
    for k in got:
        assert same_bits(got[k], runs[1][k]), "%s: two runs differ in %s" % (what, k)
    assert same_bits(got["out"], ops["out"]), "%s: Out is not written back" % what
    assert same_bits(got["g"], ops["g"]) and same_bits(got["dot"], dot0), "%s: G is read only and rowdot is ignored" % what
    for k in ("x", "r", "rs", "p"):
        assert np.array_equal(got[k], want[k]), "%s: %s: %s" % (what, k, RC.describe(got[k], want[k]))
    check_planted(case, ops, got, what)


# ------------------------------------------------------------------------------------------------ refusals
def refusals(ctx):
    """Every refused call leaves Out, the four results, G, rowdot and every guard as they were; rows == 0 is OK with NULL pointers."""
    rows, wide = 4, 257
    rng = np.random.default_rng(5)
    host = dict(out=ints(rng, 4, (rows, wide)), g=ints(rng, 4, (wide, wide)), x=ints(rng, 4, (rows, wide)), r=ints(rng, 4, (rows, wide)),
                p=ints(rng, 4, (rows, wide)), rs=np.arange(1.0, rows + 1), dot=np.full(rows, SENTINEL))
    b = Buffers(ctx, host)
    P = b.ptr
    full = lambda: K.GramCg(P("x"), P("r"), P("p"), P("rs"))

    def without(member):
        cg = full()
        setattr(cg, member, None)
        return cg

    attempts = [("Out aliases X", (P("p"), P("p"), P("g"), rows, 8, P("dot"), None)),
                ("Out aliases X", (P("p"), P("p"), P("g"), rows, 8, P("dot"), full())),
                ("null pointer", (P("out"), P("p"), None, rows, 8, P("dot"), None)),
                ("null pointer", (P("out"), P("p"), None, rows, 8, P("dot"), full())),
                ("wider than HNH_GRAM_MAX_R", (P("out"), P("p"), P("g"), rows, wide, P("dot"), full()))]
    attempts += [("null pointer in hnh_gram_cg", (P("out"), P("p"), P("g"), rows, 8, P("dot"), without(m))) for m in ("x", "r", "p", "rs")]
    for text, args in attempts:
        rc = call(ctx, *args)
        message = ctx.lib.hnh_last_error(ctx.h).decode()
        assert rc == INVALID and text in message, (rc, text, message)
        got = b.fetch("refused: " + text)
        for k in host:
            assert same_bits(got[k], host[k]), "a refused call (%s) wrote %s" % (text, k)
    for cg in (None, K.GramCg(None, None, None, None)):
        assert call(ctx, None, None, None, 0, 8, None, cg) == K.OK, "rows == 0: nothing to do, nothing to refuse"
    got = b.fetch("rows == 0")
    for k in host:
        assert same_bits(got[k], host[k])
    b.free()
    return len(attempts)


# ------------------------------------------------------------------------------------------------ the operator
OPERATOR_WIDTHS = [("hub", R, p, 1) for R in (16, 32, 64) for p in (1, 4)] + [("hub", 48, 4, 2)]
DEAD_R, DEAD_P = 64, 8            # the instance no older test launches; M = 1100 and N = 2100 leave padding rows on 8 ranks
EMPTY_USER, EMPTY_ITEM = 7, 11    # tests/als_common.py: graph("hub") keeps this row and this column empty
ZERO_W = ("hub", 64, 4, 1)


def _frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _expected(case):
    a, b, losses = IR.run(case["rows"], case["cols"], case["w"], case["A"], case["B"], IR.LAMBDA, IC.STEPS, IC.ITERS)
    return _frozen(dict(A=a, B=b, losses=losses, gramA=a.T @ a, gramB=b.T @ b))


@functools.lru_cache(maxsize=None)
def dead_rows_case():
    """hub at DEAD_R with the factor rows of the empty user and of the empty item at zero: (case, the definition's answer)"""
    base = IR.inputs("hub", DEAD_R)
    assert not np.any(base["rows"] == EMPTY_USER) and not np.any(base["cols"] == EMPTY_ITEM)
    a, b = base["A"].copy(), base["B"].copy()
    a[EMPTY_USER], b[EMPTY_ITEM] = 0.0, 0.0
    case = _frozen(dict(base, A=a, B=b, name="hub_r%d_dead_rows" % DEAD_R))
    want = _expected(case)
    assert not want["A"][EMPTY_USER].any() and not want["B"][EMPTY_ITEM].any(), "rhs = 0, M(0) = 0, rs = 0: the definition keeps them at zero"
    return case, want


@functools.lru_cache(maxsize=None)
def zero_weight_case():
    """ZERO_W with every third stored pair's weight exactly 0 (set_confidence allows w >= 0): (case, the definition's answer)"""
    base = IR.inputs(ZERO_W[0], ZERO_W[1])
    w = base["w"].copy()
    w[::3] = 0.0
    case = _frozen(dict(base, w=w, name="hub_r%d_zero_weights" % ZERO_W[1]))
    return case, _expected(case)


def run_widths(case, kind):
    """One case of OPERATOR_WIDTHS on the loaded backend: composed (and folded where the backend has the kernel) against the definition at
    T.TOL inside IC.run_case, folded against composed at T.TOL"""
    g, R, p, c = case
    composed = IC.run_case(g, R, p, c, folded=False)
    want = IR.expected(g, R)
    worst = max(T.rel(composed[k], want[k]) for k in composed)
    diff = None
    if kind == "gpu":
        folded = IC.run_case(g, R, p, c, folded=True)
        worst = max(worst, max(T.rel(folded[k], want[k]) for k in folded))
        diff = max(T.rel(folded[k], composed[k]) for k in folded)
        print("gram widths %s: folded against composed %.2e" % (case, diff))
        assert diff <= T.TOL
    T.record_observed("gram_operator_widths", case="%s R%d" % (g, R), ranks=p, c=c, worst=worst, folded_vs_composed=diff)
    return worst, diff


def run_dead_rows(folded):
    """Two steps of two iterations on DEAD_P ranks; the whole local blocks come back: padding rows and the two zeroed rows exactly zero in
    both factors, everything finite, the valid rows the definition's at T.TOL"""
    case, want = dead_rows_case()
    m, n, R = case["M"], case["N"], case["R"]
    got, per_rank = IC.run_inputs(case, want, DEAD_P, 1, folded)
    padding = 0
    for o in per_rank:
        for name, which, valid in (("A", "subA", m), ("B", "subB", n)):
            assert np.all(np.isfinite(o[name])), "a non-finite value in a local block of %s" % name
            flat, off = o[name].reshape(-1), 0
            for top, left, rc, cc in o[which]:
                blk = flat[off:off + rc * cc].reshape(rc, cc)
                off += rc * cc
                keep = max(0, min(rc, valid - top))
                padding += rc - keep
                assert not blk[keep:].any(), "padding rows of %s must stay exactly zero" % name
            assert off == flat.size
    assert padding >= 2, "the case must have padding rows on both sides"
    assert not got["A"][EMPTY_USER].any() and not got["B"][EMPTY_ITEM].any(), "rows without residual stay exactly zero"
    worst = max(T.rel(got[k], want[k]) for k in got)
    T.record_observed("gram_operator_dead_rows", case=case["name"], ranks=DEAD_P, folded=folded, worst=worst)
    return worst


def run_zero_weights(folded):
    case, want = zero_weight_case()
    assert (case["w"] == 0).sum() >= len(case["w"]) // 3 and case["w"].max() > 2
    got, _ = IC.run_inputs(case, want, ZERO_W[2], ZERO_W[3], folded)
    worst = max(T.rel(got[k], want[k]) for k in got)
    T.record_observed("gram_operator_zero_weights", case=case["name"], ranks=ZERO_W[2], folded=folded, worst=worst)
    return worst
