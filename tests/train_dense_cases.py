"""What tests/test_train_dense_instances_cpu.py and tests/test_train_dense_instances_gpu.py share (not itself a test): the case tables, a
Python restatement of every dispatcher, the operands, the host models and the guarded calls of the dense kernels of the GAT's training
path — layer normalisation (csrc/hip/hnh_gat_norm_kernels.hpp), the column sums, the skip gradient and the addend
(hnh_gat_skip_kernels.hpp), act_grad_cols_kernel (hnh_grad.hip), the optimizer steps (hnh_train_kernels.hpp, hnh_train_clip_kernels.hpp)
and the sum of squares — on the pattern of tests/dense_cases.py, whose Buffers, ints and padded are used here, with Guarded, PATTERN and
same_bits of tests/row_pass_cases.py, NormCase of tests/test_gat_norm_gpu.py and OptimProblem / ClipProblem / run_sumsq / sumsq_case of
tests/test_gat_train_gpu.py and tests/test_gat_clip_gpu.py.

THE RESTATEMENTS.  norm_instance_of(cols, vec) is norm_shape() with HNH_NORM_LAUNCH's choice: (W, T, BLOCK, lpr_log2).  norm_plan(rows,
cols) is norm_bwd_plan(): (ranges, per), at most NORM_RANGES = 1024 ranges of at least 256 rows (cols <= 512) or 16 rows.  colsum_plan(rows)
is colsum_plan(): at most COLSUM_RANGES = 512 ranges of at least 256 rows.  lane_group(cols, vec) is the group choice of
hnh_act_grad_cols_f64 and hnh_skip_grad_cols_f64: (W, lpr_log2), a trip loop beyond 64 lanes.  sumsq_blocks(units) and
optim_blocks(elements) are the workgroup counts of a tensor's run in grad_sumsq_kernel (at most 2048, 8 units per thread below the cap)
and of gridDim.x in the optimizer steps (at most 1024).  The CPU file pins each of them: against the stated instance tables, and the plans
against the workspace functions of the device library.

EXACT ARITHMETIC.  Layer norm: every row holds +1 in half of its columns and -1 in the other half (per-row permutation), or 3 +- 1, with
eps = 3: the row sum is 0 (3 cols), mu 0 (3), the squared deviations sum to cols, var + eps = 4, rstd = 0.5 and its Newton step leaves it
there, in every order of addition.  gamma = 2 h with h in {0.25, 0.5, 1}, beta = h e with e in {-2, 0, 2}: y = h (+-1 + e) is never 0;
under identity and relu out is exact, x = +-0.5, its low part 0, dY = G or 0, and with integer G of [-4, 4] dgamma and dbeta are exact sums
of multiples of 0.5, compared with an int64 model.  ELU and dz (whose means divide by cols) stay on the bounds of test_gat_norm_gpu.py.
The column sums, the two gradient kernels (identity, relu), the addend, SGD with power-of-two hyper-parameters and the sum of squares
run on small integers: every partial sum is an integer (or a dyadic fraction) far below 2^53 and every comparison is one of bit patterns.
exact_sum() asserts that on the sums of absolute values; dyadic() asserts it on every intermediate of the SGD model."""
import ctypes as C
import functools

import numpy as np

import dense_cases as D
import gat_clip_ref as CR
import gat_norm_ref as N
import gat_ref as R
import hnh_testlib as T
import row_pass_cases as RC
import test_gat_norm_gpu as NG
from distributed_sddmm_amd import _kernels as K
from row_pass_cases import PATTERN, Guarded, same_bits  # noqa: F401
from test_gat_clip_gpu import ClipProblem, run_sumsq, sumsq_case  # noqa: F401
from test_gat_train_gpu import GUARD, OptimProblem

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
BLOCK = 256
ACTS3 = ("relu", "elu", "identity")


def exact_sum(abs_sums, unit=1.0):
    """sums of absolute values, which bound every partial sum in every order: multiples of `unit` below 2^53 units"""
    a = np.asarray(abs_sums, dtype=np.float64) / unit
    assert np.all(a == np.rint(a)) and (a.size == 0 or a.max() < 2.0 ** 53), "a sum leaves the range the exactness argument covers"


def dyadic(x, bits=20):
    """multiples of 2^-bits below 2^bits: at most 2 * bits + 1 significant bits, so the operation that gave x did not round"""
    s = np.asarray(x) * 2.0 ** bits
    assert np.all(s == np.rint(s)) and (s.size == 0 or np.abs(s).max() < 2.0 ** (2 * bits)), "the SGD model leaves the exact range"
    return x


# ------------------------------------------------------------------------------------------------ the dispatchers, restated
NORM_WAVE_TRIPS, NORM_RANGES, NORM_NARROW, NORM_NARROW_ROWS, NORM_WIDE_ROWS = 4, 1024, 512, 256, 16
COLSUM_RANGES, COLSUM_MIN_ROWS, COLSUM_LANES = 512, 256, 32
SUMSQ_UNITS_PER_THREAD, SUMSQ_MAX_BLOCKS, OPTIM_MAX_BLOCKS = 8, 2048, 1024
EW_CAP = D.PLAIN_CAP


def norm_instance_of(cols, vec):
    """norm_shape() of hnh_gat_norm_kernels.hpp: (W, T, BLOCK, lpr_log2) of both layernorm kernels"""
    w = 2 if vec else 1
    block = cols > 64 * w * NORM_WAVE_TRIPS
    lpr_log2, lanes = 0, BLOCK
    if not block:
        while lpr_log2 < 6 and (w << lpr_log2) < cols:
            lpr_log2 += 1
        lanes = 1 << lpr_log2
    t = 1
    while lanes * w * t < cols:
        t *= 2
    return w, t, block, lpr_log2


def _plan(rows, least, cap):
    n = max(1, min(-(-rows // least), cap))
    per = -(-rows // n) if rows > 0 else 0
    return (-(-rows // per) if rows > 0 else 1), per


def norm_plan(rows, cols):
    """norm_bwd_plan(): (ranges, rows per range)"""
    return _plan(rows, NORM_NARROW_ROWS if cols <= NORM_NARROW else NORM_WIDE_ROWS, NORM_RANGES)


def colsum_plan(rows):
    """colsum_plan() of hnh_gat_skip_kernels.hpp: (ranges, rows per range)"""
    return _plan(rows, COLSUM_MIN_ROWS, COLSUM_RANGES)


def lane_group(cols, vec):
    """(W, lpr_log2) of act_grad_cols_kernel and skip_grad_cols_kernel: the smallest power-of-two group that covers the row, one wave at most"""
    w = 2 if vec else 1
    lpr_log2 = 0
    while lpr_log2 < 6 and (w << lpr_log2) < cols:
        lpr_log2 += 1
    return w, lpr_log2


def sumsq_blocks(units):
    """(workgroups of a tensor's run, the most units one thread walks)"""
    b = min(-(-units // (BLOCK * SUMSQ_UNITS_PER_THREAD)), SUMSQ_MAX_BLOCKS)
    return b, -(-units // (b * BLOCK))


def optim_blocks(elements):
    """(gridDim.x of an optimizer launch whose largest tensor has `elements`, the trips of its loop)"""
    b = min(-(-elements // BLOCK), OPTIM_MAX_BLOCKS)
    return b, -(-elements // (b * BLOCK))


# ------------------------------------------------------------------------------------------------ layer normalisation: the table
ISSUE_NORM_COLS = [3, 4, 5, 8, 16, 17, 32, 33, 65, 128, 129, 130, 257, 258, 512, 513, 514, 1024, 1025, 1026, 2048, 2049, 2050, 4095]
# 1, 2 and 64 complete the lane groups ((1, 0), (1, 1), (2, 0), (2, 5)), 64 and 256 the switch points 64 / 65 and 256 / 257 / 258
NORM_COLS = sorted(ISSUE_NORM_COLS + [1, 2, 64, 256])
# (cols, odd): an even width runs aligned (W = 2) and at the odd offset (W = 1), an odd one at the odd offset only
NORM_CASES = [(c, odd) for c in NORM_COLS for odd in ((False, True) if c % 2 == 0 else (True,))]
NORM_INSTANCES = [(2, 1, False), (2, 2, False), (2, 4, False), (1, 1, False), (1, 2, False), (1, 4, False), (2, 2, True), (2, 4, True), (2, 8, True),
                  (1, 2, True), (1, 4, True), (1, 8, True), (1, 16, True)]
# the two sides of every switch of norm_shape, per access width
NORM_SWITCHES = {2: [(128, 130), (256, 258), (512, 514), (1024, 1026), (2048, 2050)],
                 1: [(64, 65), (128, 129), (256, 257), (512, 513), (1024, 1025), (2048, 2049)]}
SEVERAL_NARROW, SEVERAL_WIDE = 600, 37  # three ranges of 200 rows (cols <= 512) and of 13 rows


def norm_vec(cols, odd):
    return cols % 2 == 0 and not odd


def norm_rows(cols, odd):
    """groups - 1, groups, groups + 1 for a wave shape (groups = 256 >> lpr_log2 rows per workgroup), 1, 2, 3 for a block shape, and one
    count that norm_plan cuts into three ranges"""
    w, t, block, lpr_log2 = norm_instance_of(cols, norm_vec(cols, odd))
    groups = 1 if block else BLOCK >> lpr_log2
    rows = [1, 2, 3] if block else [r for r in (groups - 1, groups, groups + 1) if r >= 1]
    return rows + [SEVERAL_NARROW if cols <= NORM_NARROW else SEVERAL_WIDE]


def norm_runs(cols, odd):
    """(rows, activation, shift) of one table entry: all three activations at the ragged count, one each (rotating) at the others"""
    rows = norm_rows(cols, odd)
    ragged = rows[-2]
    runs = []
    for i, r in enumerate(rows):
        for act in (ACTS3 if r == ragged else (ACTS3[(i + cols) % 3],)):
            runs.append((r, act, 1000.0 if r != ragged and i % 2 == 1 else 0.0))  # (rows of 1000 + [-1, 1] at one count per entry)
    return runs


def norm_id(case):
    return "%d%s" % (case[0], "_odd" if case[1] else "")


# rows x cols, odd, capped: norm_plan's cap with its last uncapped neighbour, wide (16 rows per range at least) and narrow (256)
NORM_CAPS = [(17000, 514, False, True), (16384, 514, False, False), (270001, 6, False, True), (270001, 6, True, True), (262144, 6, False, False)]
NORM_EXACT_EPS = 3.0


@functools.lru_cache(maxsize=2)
def norm_exact_operands(rows, cols, base):
    """(z, gamma, beta, G, s): z = base + s with s = +-1, half of each per row"""
    assert cols % 2 == 0 and base in (0.0, 3.0)
    rng = np.random.default_rng(7 * rows + cols + int(base))
    s = rng.permuted(np.tile(np.repeat([1.0, -1.0], cols // 2), (rows, 1)), axis=1)
    h = rng.choice([0.25, 0.5, 1.0], cols)
    e = rng.choice([-2.0, 0.0, 2.0], cols)
    e[:3] = [0.0, 2.0, -2.0][:min(cols, 3)]  # (a narrow row too has a column gated by the sign of s, then one always on, one always off)
    gamma, beta = 2.0 * h, h * e
    g = D.ints(rows + 3 * cols, (rows, cols))
    return base + s, gamma, beta, g, s


def norm_exact_model(rows, cols, base, act):
    """stats, out, dgamma, dbeta of the exact operands under identity or relu, the gradients from int64 sums"""
    z, gamma, beta, g, s = norm_exact_operands(rows, cols, base)
    y = gamma[None, :] * (0.5 * s) + beta[None, :]
    assert np.all(y != 0.0) and np.all(y * 4 == np.rint(y * 4)), "no y on the gate, every y a multiple of 0.25"
    on = np.ones_like(y, dtype=bool) if act == "identity" else y > 0
    out = np.where(on, y, 0.0)
    dy = np.where(on, g, 0.0).astype(np.int64)
    si = s.astype(np.int64)
    exact_sum(np.abs(dy).sum(axis=0))  # (bounds |dY x| too: |x| = 0.5)
    stats = np.column_stack([np.full(rows, base), np.full(rows, 0.5)])
    return stats, out, (dy * si).sum(axis=0) / 2.0, dy.sum(axis=0).astype(np.float64), float(np.count_nonzero(on)) / on.size


def norm_exact(ctx, rows, cols, odd, base, acts, light=False):
    """One NormCase on the exact operands.  identity / relu: stats, out, dgamma, dbeta by bit pattern; elu: stats by bit pattern, out on
    the forward bound; dz on its bound per row under every activation; repeats and in-place calls bit-equal (light: one call each).
    Returns the worst (forward, dz) shares of their bounds."""
    z, gamma, beta, g, s = norm_exact_operands(rows, cols, base)
    c = NG.NormCase(ctx, rows, cols, z, gamma, beta, g, odd, eps=NORM_EXACT_EPS)
    assert c.need == norm_plan(rows, cols)[0] * 2 * cols
    cond = 1.0 + np.abs(z).max(axis=1) * 0.5
    f_bound = 32 * EPS64 * cond * max(1.0, float(np.abs(gamma).max()))
    b_bound = 128 * EPS64 * cond * float(np.abs(g).max()) * float(np.abs(gamma).max()) * 0.5
    worst = [0.0, 0.0]
    for act in acts:
        what = "layernorm exact %dx%d odd=%s base=%s %s" % (rows, cols, odd, base, act)
        c.reset("out", "dz", "dgamma", "dbeta", "work", "stats")
        out, stats = c.forward(act)
        if act == "elu":
            want_stats = np.column_stack([np.full(rows, base), np.full(rows, 0.5)])
            want = N.ln_forward(z, gamma, beta, NORM_EXACT_EPS, act, LD)[0]
            f_err = np.max(np.abs(out.astype(LD) - want), axis=1).astype(np.float64)
            worst[0] = max(worst[0], float(np.max(f_err / f_bound)))
            assert np.all(f_err <= f_bound), (what, float(np.max(f_err / f_bound)))
        else:
            want_stats, want_out, want_dg, want_db, _ = norm_exact_model(rows, cols, base, act)
            assert same_bits(out, want_out), what + ": out: " + RC.describe(out, want_out)
        assert same_bits(stats, want_stats), what + ": stats: " + RC.describe(stats, want_stats)
        dz, dgamma, dbeta = c.backward(act)
        if act != "elu":
            assert same_bits(dgamma, want_dg), what + ": dgamma: " + RC.describe(dgamma, want_dg)
            assert same_bits(dbeta, want_db), what + ": dbeta: " + RC.describe(dbeta, want_db)
        want_dz = N.ln_backward(g, z, gamma, beta, NORM_EXACT_EPS, act, LD)[0]
        b_err = np.max(np.abs(dz.astype(LD) - want_dz), axis=1).astype(np.float64)  # (a row no range owns keeps NormCase's fill of 5 .. 6)
        worst[1] = max(worst[1], float(np.max(b_err / b_bound)))
        assert np.all(b_err <= b_bound), (what, "dz", float(np.max(b_err / b_bound)), int(np.argmax(b_err / b_bound)))
        if light:
            continue
        out2, stats2 = c.forward(act)
        dz2, dgamma2, dbeta2 = c.backward(act)
        assert same_bits(out, out2) and same_bits(stats, stats2) and same_bits(dz, dz2) and same_bits(dgamma, dgamma2) and same_bits(dbeta, dbeta2), \
            what + ": a repeat must be bit-identical"
        dz3, dgamma3, dbeta3 = c.backward(act, in_place=True)
        assert same_bits(dz, dz3) and same_bits(dgamma, dgamma3) and same_bits(dbeta, dbeta3), what + ": dz == G is bit-equal to out of place"
        c.reset("stats")
        out3, stats3 = c.forward(act, in_place=True)
        assert same_bits(out, out3) and same_bits(stats, stats3), what + ": out == z is bit-equal to out of place"
        c.reset("g", "z")
    c.free()
    return tuple(worst)


# ------------------------------------------------------------------------------------------------ hnh_colsum_f64
COLSUM_COLS = [1, 2, 31, 32, 33, 63, 64, 65, 66, 130]
COLSUM_ROWS = [1, 7, 8, 9, 255, 256, 257, 513]
COLSUM_CASES = [(c, moved) for c in COLSUM_COLS for moved in (False, True)]
COLSUM_CAPS = [(150001, 6, True), (150001, 5, True), (131072, 6, False)]  # rows, cols, capped


def colsum_width(cols, moved):
    """W of colsum_ranges_kernel at the pitch cols + 2"""
    return 2 if cols % 2 == 0 and not moved else 1


def colsum_data(rows, cols):
    a = D.ints(131 * rows + cols, (rows, cols))
    exact_sum(np.abs(a).sum(axis=0))
    return a, a.astype(np.int64).sum(axis=0).astype(np.float64)


def colsum(ctx, rows, cols, moved=False):
    """src at pitch cols + 2 with NaN pad columns, out and the workspace (at exactly hnh_colsum_f64_workspace doubles) between guards"""
    a, want = colsum_data(rows, cols)
    ld = cols + 2
    need = int(ctx.lib.hnh_colsum_f64_workspace(rows, cols))
    assert need == colsum_plan(rows)[0] * cols
    with D.Buffers(ctx) as bufs:
        ps = bufs.add("src", D.padded(a, ld), moved)
        po, pw = bufs.add("out", np.full(cols, 9.0)), bufs.add("work", np.full(need, 5.0), scratch=True)
        for rnd in range(2):
            bufs.a["out"].set(np.full(cols, 9.0 + rnd))
            ctx.check(ctx.lib.hnh_colsum_f64(ctx.h, po, ps, ld, rows, cols, pw, need, K.STREAM_COMPUTE), "hnh_colsum_f64")
            bufs.verify("colsum %dx%d moved=%s run %d" % (rows, cols, moved, rnd), out=want)
    return want


# ------------------------------------------------------------------------------------------------ the two gradient kernels
ISSUE_GRAD_WIDTHS = [2, 4, 5, 8, 16, 17, 32, 33, 65, 128, 129, 130]
GRAD_WIDTHS = sorted(ISSUE_GRAD_WIDTHS + [1, 64])  # (1 and 64 complete the groups: (1, 0) and (2, 5))
GRAD_CASES = [(f, even) for f in GRAD_WIDTHS for even in (True, False)]
EXACT_ACTS = ("identity", "relu")
SKIP_SWITCHES = [(r, b, a) for r in (False, True) for b in (False, True) for a in (False, True)]  # res, bias, dZ_all


def grad_vec(f, even):
    return even and f % 2 == 0


def grad_rows(f, even):
    groups = BLOCK >> lane_group(f, grad_vec(f, even))[1]
    return [r for r in (groups - 1, groups, groups + 1) if r >= 1]


def grad_id(case):
    return "f%d_%s" % (case[0], "even" if case[1] else "odd")


def grad_layout(f, even):
    """the siblings' layout (act_grad_case): three heads of f columns, the middle one the call's; every pitch even or every pitch odd"""
    col0 = f + (f & 1) if even else f
    fix = (lambda v: v + v % 2) if even else (lambda v: v + 1 - v % 2)
    return dict(col0=col0, ld_g=fix(col0 + f + 4), ld_o=fix(col0 + f + 6), ld_dz=fix(f + 2), ld_all=fix(col0 + f + 8), ld_r=fix(f + 2))


def grad_operands(rows, f, even):
    lay = grad_layout(f, even)
    wide = lay["col0"] + f
    seed = 1000 * rows + 10 * f + even
    g, o = D.ints(seed, (rows, wide)), D.ints(seed + 1, (rows, wide), zeros=0.1)
    res, bias = D.ints(seed + 2, (rows, f)), D.ints(seed + 3, f)
    return lay, g, o, res, bias


def grad_model(g, o, act, addend):
    """dZ and delta of the middle head's block (g, o: that block): integers"""
    out = np.maximum(o, 0.0) if act == "relu" else o
    on = out > 0 if act == "relu" else np.ones_like(out, dtype=bool)
    dz = np.where(on, g, 0.0)
    terms = np.where(on, g * (out - addend), 0.0)
    exact_sum(np.abs(terms).sum(axis=1))
    return out, RC.exact(dz), RC.exact(terms.sum(axis=1) + 0.0)


def act_grad(ctx, rows, f, even):
    """hnh_act_grad_cols_f64 under identity and relu, exactly: G and out with NaN pad columns, dZ inside 7.0, delta, all between guards"""
    lay, g, o, _, _ = grad_operands(rows, f, even)
    col0 = lay["col0"]
    with D.Buffers(ctx) as bufs:
        pg = bufs.add("G", D.padded(g, lay["ld_g"]))
        po = bufs.add("out", D.padded(o, lay["ld_o"]))
        pz, pd = bufs.add("dZ", np.full((rows, lay["ld_dz"]), 7.0)), bufs.add("delta", np.full(rows, 9.0))
        for act in EXACT_ACTS:
            out, dz, delta = grad_model(g[:, col0:], o[:, col0:], act, 0.0)
            full = o.copy()
            full[:, col0:] = out
            bufs.a["out"].set(D.padded(full, lay["ld_o"]))
            bufs.a["dZ"].set(np.full((rows, lay["ld_dz"]), 7.0))
            bufs.a["delta"].set(np.full(rows, 9.0))
            ctx.check(ctx.lib.hnh_act_grad_cols_f64(ctx.h, pz, lay["ld_dz"], pd, pg, lay["ld_g"], po, lay["ld_o"], col0, rows, f, R.ACT_CODE[act],
                                                    K.STREAM_COMPUTE), "hnh_act_grad_cols_f64")
            want = np.full((rows, lay["ld_dz"]), 7.0)
            want[:, :f] = dz
            bufs.verify("act_grad %dx%d even=%s %s" % (rows, f, even, act), dZ=want, delta=delta)
    return dz, delta


def skip_grad(ctx, rows, f, even):
    """hnh_skip_grad_cols_f64 under identity and relu with every choice of res, bias and dZ_all, exactly"""
    lay, g, o, res, bias = grad_operands(rows, f, even)
    col0 = lay["col0"]
    with D.Buffers(ctx) as bufs:
        pg, po = bufs.add("G", D.padded(g, lay["ld_g"])), bufs.add("out", D.padded(o, lay["ld_o"]))
        pr, pb = bufs.add("res", D.padded(res, lay["ld_r"])), bufs.add("bias", bias)
        pz, pa = bufs.add("dZ", np.full((rows, lay["ld_dz"]), 7.0)), bufs.add("dZ_all", np.full((rows, lay["ld_all"]), 6.0))
        pd = bufs.add("delta", np.full(rows, 9.0))
        for act in EXACT_ACTS:
            for use_res, use_bias, use_all in SKIP_SWITCHES:
                addend = (res if use_res else 0.0) + (bias[None, :] if use_bias else 0.0)
                out, dz, delta = grad_model(g[:, col0:], o[:, col0:], act, addend)
                full = o.copy()
                full[:, col0:] = out
                bufs.a["out"].set(D.padded(full, lay["ld_o"]))
                bufs.a["dZ"].set(np.full((rows, lay["ld_dz"]), 7.0))
                bufs.a["dZ_all"].set(np.full((rows, lay["ld_all"]), 6.0))
                bufs.a["delta"].set(np.full(rows, 9.0))
                rc = ctx.lib.hnh_skip_grad_cols_f64(ctx.h, pz, lay["ld_dz"], pa if use_all else None, lay["ld_all"], pd, pg, lay["ld_g"], po, lay["ld_o"], col0,
                                                    pr if use_res else None, lay["ld_r"], pb if use_bias else None, rows, f, R.ACT_CODE[act], K.STREAM_COMPUTE)
                ctx.check(rc, "hnh_skip_grad_cols_f64")
                want, want_all = np.full((rows, lay["ld_dz"]), 7.0), np.full((rows, lay["ld_all"]), 6.0)
                want[:, :f] = dz
                if use_all:
                    want_all[:, col0:col0 + f] = dz
                bufs.verify("skip_grad %dx%d even=%s %s res=%s bias=%s all=%s" % (rows, f, even, act, use_res, use_bias, use_all), dZ=want, dZ_all=want_all,
                            delta=delta)


# ------------------------------------------------------------------------------------------------ hnh_skip_addend_cols_f64 past ew_grid's cap
# rows, cols, pitch of dst, col0 -> W: 246 739 x 17 is exactly D.PAST_PLAIN items (two full trips and 259 more); x 34 at an even col0 the same
# number of 16-byte items, at an odd col0 twice as many 8-byte ones
ADDEND_PAST = {(D.PAST_COLS[0], 17, 22, 2): 1, (D.PAST_COLS[0], 34, 38, 2): 2, (D.PAST_COLS[0], 34, 38, 3): 1}


def addend_id(case):
    return "%dx%d_ld%d_col%d" % case


def skip_addend(ctx, rows, cols, ld, col0):
    """dst (integers, rows x ld) gets res + bias, res, bias or +0.0 in its columns col0 .. col0 + cols; everything else and the guards stay"""
    dst0, res, bias = D.ints(41, (rows, ld)), D.ints(42, (rows, cols)), D.ints(43, cols)
    exact_sum(np.abs(res) + np.abs(bias)[None, :])
    with D.Buffers(ctx) as bufs:
        pd, pr, pb = bufs.add("dst", dst0), bufs.add("res", res), bufs.add("bias", bias)
        for use_res in (True, False):
            for use_bias in (True, False):
                bufs.a["dst"].set(dst0)
                ctx.check(ctx.lib.hnh_skip_addend_cols_f64(ctx.h, pd, ld, col0, pr if use_res else None, cols, pb if use_bias else None, rows, cols,
                                                           K.STREAM_COMPUTE), "hnh_skip_addend_cols_f64")
                want = dst0.copy()
                want[:, col0:col0 + cols] = RC.exact((res if use_res else 0.0) + (bias[None, :] if use_bias else 0.0) + np.zeros((rows, cols)))
                bufs.verify("skip_addend %s res=%s bias=%s" % ((rows, cols, ld, col0), use_res, use_bias), dst=want)


# ------------------------------------------------------------------------------------------------ the optimizer steps past 1024 workgroups
OPTIM_BIG = (1025, 257, 259)  # rows, cols, pitch: 263 425 elements, a full trip of 262 144 and 1281 more
# (rows, cols, pad of the parameter's pitch): the big tensor among tensors of 1, 255, 256, 257 and 262 144 elements in the first launch of 32;
# the rest of the table is a second launch of small tensors alone
OPTIM_TABLE = [(1, 1, 0), (1, 255, 1), (256, 1, 0), (257, 1, 2), OPTIM_BIG[:2] + (2,), (512, 512, 0)] + \
              [((1, 255, 0), (16, 16, 1), (1, 257, 2), (1, 1, 1))[k % 4] for k in range(26)] + [(3, 85, 1), (257, 1, 0), (1, 1, 0)]
SGD_EXACT = dict(lr=0.25, momentum=0.5, weight_decay=0.25)
CLIP_QUARTER_SUMS = [7.0, 9.0]  # norm 4: max_norm = (4 + 1e-6) / 4 makes the coefficient exactly 0.25
CLIP_QUARTER_MAX_NORM = (np.sqrt(16.0) + 1e-6) / 4.0


class PastCapOptim(ClipProblem):
    """OptimProblem / ClipProblem over OPTIM_TABLE: every tensor with a gradient of its own at pitch cols + (0, 1, 2), the parameter's
    pitch padding holding GUARD.  integer=True: p, g and v are integers of [-4, 4] and new_gradients() draws new integers."""

    def __init__(self, ctx, kind, integer=False, seed=0):
        self.ctx, self.kind, self.integer = ctx, kind, integer
        self.rng = np.random.default_rng(seed)
        self.tensors, self.dev = [], []
        for k, (rows, cols, pad) in enumerate(OPTIM_TABLE):
            gpad = k % 3
            p = self.array(np.where(np.arange(cols + pad) < cols, self.draw((rows, cols + pad)), GUARD))
            self.add(p, cols + pad, self.array(self.draw((rows, cols + gpad))), min(gpad, 1), cols + gpad, rows, cols)
            if integer:
                t = self.tensors[-1]
                t["v"]["host"] = self.draw((rows, cols))
                t["v"]["dev"].set(t["v"]["host"])
        assert K.OPTIM_MAX_TENSORS < len(self.tensors) < 2 * K.OPTIM_MAX_TENSORS

    def draw(self, shape):
        return self.rng.integers(-4, 5, shape).astype(np.float64) if self.integer else self.rng.standard_normal(shape)

    def new_gradients(self):
        if not self.integer:
            return OptimProblem.new_gradients(self)
        for t in self.tensors:
            t["g"]["host"] = self.draw(t["g"]["host"].shape)
            t["g"]["dev"].set(t["g"]["host"])

    def exact_sgd_step(self, entry, coef=1.0, sums=None, max_norm=0.0):
        """one SGD step of SGD_EXACT through hnh_optim_step_f64 ("plain") or hnh_optim_step_clip_f64 ("clip"), then every p and v by bit
        pattern against the host model, whose every intermediate is asserted dyadic (so no operation of it rounded, fused or not)"""
        assert self.integer and self.kind == "sgd"
        if entry == "plain":
            hy = self.hyper(1, SGD_EXACT)
            self.ctx.check(self.ctx.lib.hnh_optim_step_f64(self.ctx.h, self.table(), len(self.tensors), C.byref(hy), K.STREAM_COMPUTE), "hnh_optim_step_f64")
            self.ctx.sync()
        else:
            self.clip_step(1, SGD_EXACT, sums, max_norm)
        lr, mom, wd = SGD_EXACT["lr"], SGD_EXACT["momentum"], SGD_EXACT["weight_decay"]
        for k, t in enumerate(self.tensors):
            cols = t["cols"]
            p = t["p"]["host"][:, :cols]
            g = dyadic(coef * t["g"]["host"][:, t["g_off"]:t["g_off"] + cols])
            gd = dyadic(g + dyadic(wd * p))
            v = dyadic(dyadic(mom * t["v"]["host"]) + gd)
            newp = dyadic(p - dyadic(lr * v))
            t["v"]["host"], t["p"]["host"][:, :cols] = v, newp
            got_p, got_v = t["p"]["dev"].get(), t["v"]["dev"].get()
            assert np.all(got_p[:, cols:] == GUARD), "the parameter's pitch padding is untouched"
            assert same_bits(np.ascontiguousarray(got_p[:, :cols]), np.ascontiguousarray(newp)), "tensor %d p: %s" % (k, RC.describe(got_p[:, :cols], newp))
            assert same_bits(got_v, v), "tensor %d v: %s" % (k, RC.describe(got_v, v))
            assert np.array_equal(t["g"]["dev"].get(), t["g"]["host"]), "the gradient is read, never written"

    def clip_step_checked(self, step, hyper, sums, max_norm):
        """ClipProblem.clip_step and the comparison of test_clip_step_kernel_vs_numpy: against gat_ref / gat_clip_ref at T.TOL"""
        coef = min(1.0, max_norm / (np.sqrt(sum(sums)) + 1e-6)) if sums else 1.0
        self.clip_step(step, hyper, sums, max_norm)
        worst = 0.0
        for t in self.tensors:
            cols = t["cols"]
            g = coef * t["g"]["host"][:, t["g_off"]:t["g_off"] + cols]
            old = t["p"]["host"][:, :cols]
            kw = {k: hyper[k] for k in ("beta1", "beta2", "eps", "weight_decay") if k in hyper}
            newp, t["m"]["host"], t["v"]["host"] = (R.adam_step if self.kind == "adam" else CR.adamw_step)(old, g, t["m"]["host"], t["v"]["host"], step, hyper["lr"], **kw)
            t["p"]["host"][:, :cols] = newp
            got_p = t["p"]["dev"].get()
            assert np.all(got_p[:, cols:] == GUARD), "the parameter's pitch padding is untouched"
            errs = [T.rel(got_p[:, :cols], newp), T.rel(t["v"]["dev"].get(), t["v"]["host"]), T.rel(t["m"]["dev"].get(), t["m"]["host"])]
            worst = max(worst, *errs)
            assert max(errs) <= T.TOL, (step, t["rows"], cols, t["ld_g"], errs)
        return worst


def optim_exact_sgd(ctx, entry, coef=1.0, steps=3):
    """three exact SGD steps with new integer gradients; "clip": coef 1 from sums far below max_norm, or exactly 0.25"""
    p = PastCapOptim(ctx, "sgd", integer=True, seed=5)
    sums, max_norm = (None, 0.0) if entry == "plain" else (([1.0, 3.0], 1e6) if coef == 1.0 else (CLIP_QUARTER_SUMS, CLIP_QUARTER_MAX_NORM))
    start = [t["p"]["host"].copy() for t in p.tensors]
    for _ in range(steps):
        p.exact_sgd_step(entry, coef, sums, max_norm)
        p.new_gradients()
    moved = sum(bool(np.any(t["p"]["host"] != s)) for t, s in zip(p.tensors, start))
    p.free()
    assert moved >= len(start) - 3, "every tensor has moved (a one-element tensor may come back to its start)"


def optim_adam(ctx, steps=2):
    """hnh_optim_step_f64 with Adam over OPTIM_TABLE against gat_ref.adam_step at T.TOL (OptimProblem.step asserts it)"""
    p = PastCapOptim(ctx, "adam", seed=6)
    worst = 0.0
    for step in range(1, steps + 1):
        worst = max(worst, p.step(step, dict(lr=0.01, weight_decay=5e-4)))
        p.new_gradients()
    p.free()
    return worst


def optim_clip(ctx, kind, steps=2):
    """hnh_optim_step_clip_f64 with Adam or AdamW over OPTIM_TABLE, a coefficient of about 0.25, against gat_clip_ref at T.TOL"""
    p = PastCapOptim(ctx, kind, seed=7)
    worst = 0.0
    for step in range(1, steps + 1):
        worst = max(worst, p.clip_step_checked(step, dict(lr=0.01, weight_decay=0.01), [30.0, 6.0], 1.5))
        p.new_gradients()
    p.free()
    return worst


# ------------------------------------------------------------------------------------------------ hnh_grad_sumsq_f64 past 2048 workgroups
# name -> (rows, cols, pitch, moved): a dense even tensor of 8 391 076 doubles (units of two, 4 195 538 of them: a ninth unit in some
# threads) aligned and moved by one double; a pitched one of 4 200 003 units of one double, capped, 174 762 rows a step; one whose rows
# are wider than the run's threads (1026 workgroups: step_r == 0)
SUMSQ_BIG = {"dense": (2, 4195538, 4195538, False), "dense_moved": (2, 4195538, 4195538, True), "pitched": (1400001, 3, 4, False),
             "long_rows": (3, 700001, 700002, False)}


def sumsq_units(rows, cols, pitch):
    """(doubles in a unit, units in a row, units in all) of sumsq_plan()"""
    dense = pitch == cols or rows == 1
    width = rows * cols if dense else cols
    unit = 2 if width % 2 == 0 else 1
    return unit, width // unit, rows * cols // unit


def sumsq_big(ctx, name):
    """(the guarded device array, its table entry, the int64 sum of squares); integers of [-8, 8], the pad columns NaN"""
    rows, cols, pitch, moved = SUMSQ_BIG[name]
    a = D.ints(rows + cols, (rows, cols), k=8)  # (the aligned and the moved dense tensor hold the same numbers)
    want = int(np.square(a.astype(np.int64)).sum())
    assert want < 2 ** 53
    g = Guarded(ctx, D.padded(a, pitch), int(moved), name)
    return g, K.OptimTensor(None, 0, g.ptr, pitch, None, None, rows, cols), want


def sumsq_checked(ctx, tab, n, guarded, want, accumulate=0, start=GUARD):
    got = run_sumsq(ctx, tab, n, accumulate, start)
    for g in guarded:
        inner, ok = g.fetch()
        assert ok and same_bits(inner, g.host), "the gradient %s is read, never written, and its guards hold" % g.name
    assert got == float(want) + (start if accumulate else 0.0), (got, want)
    return got
