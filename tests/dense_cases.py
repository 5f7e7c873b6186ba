"""What tests/test_dense_instances_cpu.py and tests/test_dense_instances_gpu.py share (not itself a test): the case tables, the integer
data, the numpy model and the guarded calls of the dense side of include/hnh_kernels.h and include/hnh_grad.h — both MFMA GEMMs, the
ALS row helpers and the streaming element-wise kernels — on the pattern of tests/row_pass_cases.py, whose Guarded, PATTERN, same_bits
and DoubleCtx are used here.

EXACT ARITHMETIC.  Matrices are integers of [-4, 4]; scalars and row factors are powers of two (0.25, +-0.5, +-1, +-2); divisors are
powers of two.  Every product and every partial sum is then a multiple of 2^-4 whose magnitude stays below SUM_BOUND = 16 * 32769 (the
longest sum has 32769 terms of at most 16), far below 2^53: every order of addition, fused or not, gives the same bits, and results are
compared with same_bits, never by distance.  bounded() asserts the bound on the sums of ABSOLUTE values, which bound every partial sum
in every order.  No input and no result is a negative zero (row_pass_cases.exact asserts it): LeakyReLU sees nonzero integers and +0.0,
a product whose sign could end up on a zero (Hadamard, row_scale_add's Y, a quotient) has nonzero operands.

GUARDS.  Every operand and every output (the split-K workspace too, passed at exactly the size asked for) lies between two 128-byte
guards of one quiet-NaN pattern.  After every call Buffers.verify() asserts that all guards hold, that the inputs are bit-identical to
what was uploaded and that the outputs are the model's, which includes the columns of a pitched output outside the written block.  The
pad columns of pitched INPUTS hold the NaN pattern: a read that strays into them shows in the result.  "Moved" = the pointer advanced
by one double, so 8-byte aligned only.

THE GRID CAPS.  ew_grid() launches at most 8192 blocks of 256 threads.  A plain grid-stride loop takes a second trip beyond
PLAIN_CAP = 2 097 152 items; a 4x-unrolled loop over 16-byte pairs beyond UNROLLED_CAP = 16 777 216 doubles.  PAST_PLAIN = 4 194 563
is two full trips and a third of 259 items; PAST_UNROLLED = 20 971 721 a full unrolled trip, a second one of 2 097 252 pairs (u = 0
whole, u = 1 a hundred pairs, u = 2, 3 empty) and an odd last element."""
import ctypes as C
import functools

import numpy as np

import row_pass_cases as RC
from distributed_sddmm_amd import _kernels as K
from oracle import oracle as O
from row_pass_cases import PATTERN, DoubleCtx, Guarded, same_bits

INVALID = 1
ROWS = 523                        # prime and above 2 x 256: no group size divides it, every instance runs more than two workgroups
SUM_BOUND = 16 * 32769
POW2 = np.array([0.25, -0.5, 0.5, -1.0, 1.0, -2.0, 2.0])
NAN_PAD = np.array([PATTERN]).view(np.float64)[0]
PLAIN_CAP, UNROLLED_CAP = 8192 * 256, 8192 * 256 * 2 * 4
PAST_PLAIN, PAST_UNROLLED = 4194563, 20971721
PAST_COLS = (246739, 17)          # rows x cols of the column-block kernels past the cap: exactly PAST_PLAIN items
EW_SIZES = [1, 2, 3, 7, 8, 9, 2047, 2048, 2049, 100003]
# the column-block kernels at those sizes: rows x cols with that many items (100003 is prime)
COLS_SHAPE = {1: (1, 1), 2: (1, 2), 3: (3, 1), 7: (1, 7), 8: (2, 4), 9: (3, 3), 2047: (89, 23), 2048: (64, 32), 2049: (683, 3), 100003: (100003, 1)}
TILE_PERIOD = 1000003             # prime: a large operand repeats a random block of this length, which no stride of a loop divides


class GradDoubleCtx(DoubleCtx):
    """the second double (oracle/hnh_oracle_gat_groups.h behind the same source): the mandatory table and include/hnh_grad.h"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name, (res, args) in list(K.SIGNATURES.items()) + list(K.GRAD_SIGNATURES.items()):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        assert self.lib.hnh_backend_name() == b"oracle-cpu-test-double-gat"
        h = C.c_void_p()
        assert self.lib.hnh_ctx_create(0, C.byref(h)) == K.OK
        self.h = h


# ------------------------------------------------------------------------------------------------ data and model helpers
def ints(seed, shape, zeros=0.03, k=4):
    """integers of [-k, k] as float64, a share `zeros` of them +0.0; large operands tile a random block of prime length"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if n <= 2 * TILE_PERIOD:
        return RC._ints(rng, k, shape, zeros)
    return np.resize(RC._ints(rng, k, TILE_PERIOD, zeros), n).reshape(shape)


def pow2(seed, n):
    """row factors out of POW2; beyond 1009 rows a block of that (prime) length repeats"""
    return np.resize(np.random.default_rng(seed).choice(POW2, min(n, 1009)), n)


def bounded(abs_sums):
    """the sums of absolute values, which bound every partial sum in every order: exact and at most 16 * 32769"""
    abs_sums = np.asarray(abs_sums)
    RC.exact(abs_sums)
    assert abs_sums.size == 0 or abs_sums.max() <= SUM_BOUND, "a sum leaves the range the exactness argument covers"


def padded(a, ld, fill=NAN_PAD):
    """a (rows x cols) at pitch ld, the pad columns holding `fill`"""
    out = np.full((a.shape[0], ld), fill)
    out[:, :a.shape[1]] = a
    return out


def ew_trips(n, per_trip):
    return -(-n // per_trip)


class Buffers:
    """The guarded device arrays of one call.  verify(): the guards of ALL arrays, the inputs bit for bit, the outputs against the
    model; a scratch array (the split-K workspace) is checked for its guards only."""

    def __init__(self, ctx):
        self.ctx, self.a, self.scratch = ctx, {}, set()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for g in self.a.values():
            g.free()
        return False

    def add(self, name, host, moved=False, scratch=False):
        g = Guarded(self.ctx, np.ascontiguousarray(host, dtype=np.float64), int(bool(moved)), name)
        assert g.ptr % 16 == (8 if moved else 0)
        self.a[name] = g
        if scratch:
            self.scratch.add(name)
        return g.ptr

    def verify(self, what, **outputs):
        self.ctx.sync()
        got_all = {}
        for name, arr in self.a.items():
            got, guards = arr.fetch()
            assert guards, "%s: a guard of %s was overwritten" % (what, name)
            got_all[name] = got
            if name in self.scratch:
                continue
            want = np.ascontiguousarray(outputs.get(name, arr.host), dtype=np.float64).reshape(arr.shape)
            kind = "output" if name in outputs else "input"
            assert same_bits(got, want), "%s: %s %s: %s" % (what, kind, name, RC.describe(got, want))
        assert set(outputs) <= set(self.a)
        return got_all


def refused(ctx, rc, text):
    assert rc == INVALID, rc
    got = ctx.lib.hnh_last_error(ctx.h).decode()
    assert got == text, got


# ------------------------------------------------------------------------------------------------ C = A B (hnh_gemm_f64)
GEMM_SHAPES = [(4, 3, 0), (1, 1, 1), (5, 3, 1), (127, 127, 15), (128, 128, 16), (129, 129, 17), (128, 130, 32), (256, 128, 48), (257, 128, 34),
               (255, 256, 33), (1025, 130, 18), (2049, 2, 18)]
GEMM_CASES = [s + (None,) for s in GEMM_SHAPES] + [(256, 256, 64, m) for m in ("A", "B", "C")]


def gemm_id(c):
    return "%dx%dx%d%s" % (c[0], c[1], c[2], "" if c[3] is None else "_%s_moved" % c[3])


@functools.lru_cache(maxsize=None)
def gemm_data(M, N, Kk):
    a, b = ints(11 * M + Kk, (M, Kk)), ints(13 * N + Kk + 1, (Kk, N))
    bounded(np.abs(a) @ np.abs(b))
    return a, b, RC.exact(a @ b + 0.0)


def gemm(ctx, M, N, Kk, moved=None):
    """two runs onto a prefilled C: each the model's bits (so bit-equal to each other); K = 0 passes null operands -> C"""
    a, b, want = gemm_data(M, N, Kk)
    with Buffers(ctx) as bufs:
        pa = bufs.add("A", a, moved == "A") if Kk else None
        pb = bufs.add("B", b, moved == "B") if Kk else None
        pc = bufs.add("C", np.full((M, N), 9.0), moved == "C")
        runs = []
        for rnd in range(2):
            bufs.a["C"].set(np.full((M, N), 9.0 + rnd))
            ctx.check(ctx.lib.hnh_gemm_f64(ctx.h, M, N, Kk, pa, pb, pc, 0), "gemm")
            runs.append(bufs.verify("gemm %s run %d" % ((M, N, Kk, moved), rnd), C=want)["C"])
        assert same_bits(runs[0], runs[1])
        if Kk == 0:
            assert same_bits(runs[0], np.zeros((M, N)))
        return runs[0]


def gemm_refusals(ctx):
    a, b, _ = gemm_data(5, 3, 1)
    with Buffers(ctx) as bufs:
        pa, pb, pc = bufs.add("A", a), bufs.add("B", b), bufs.add("C", np.full((5, 3), 9.0))
        for m, n, k in ((-1, 3, 1), (5, -1, 1), (5, 3, -1)):
            refused(ctx, ctx.lib.hnh_gemm_f64(ctx.h, m, n, k, pa, pb, pc, 0), "hnh_gemm_f64: negative size")
        for ops in ((None, pb, pc), (pa, None, pc), (pa, pb, None)):
            refused(ctx, ctx.lib.hnh_gemm_f64(ctx.h, 5, 3, 1, *ops, 0), "hnh_gemm_f64: null pointer")
        refused(ctx, ctx.lib.hnh_gemm_f64(ctx.h, 5, 3, 0, None, None, None, 0), "hnh_gemm_f64: null pointer")
        bufs.verify("refused gemm calls")
        ctx.check(ctx.lib.hnh_gemm_f64(ctx.h, 0, 3, 1, None, None, None, 0), "M = 0")
        ctx.check(ctx.lib.hnh_gemm_f64(ctx.h, 5, 0, 1, None, None, None, 0), "N = 0")
        bufs.verify("empty gemm calls")


# ------------------------------------------------------------------------------------------------ C = A^T B (hnh_gemm_tn_f64)
def tn_plan(M, N, Kk):
    """tn_plan of csrc/hip/hnh_grad.hip restated: (slices, K rows per slice)"""
    tiles, kt = -(-M // 128) * -(-N // 128), -(-Kk // 16)
    s = 1
    if 0 < tiles < 512:
        s = max(1, min(-(-512 // tiles), kt // 32, 64))
    per = -(-kt // s) if kt > 0 else 1
    return (-(-kt // per) if kt > 0 else 1), per * 16


def tn_workspace(M, N, Kk):
    if M <= 0 or N <= 0 or Kk <= 0:
        return 0
    s = tn_plan(M, N, Kk)[0]
    return s * M * N if s > 1 else 0


# (M, N, K, pad) -> the slices the issue states for it
TN_SLICES = {(16, 8, 1, 3): 1, (1, 1, 1008, 0): 1, (1, 1, 1009, 0): 2, (17, 9, 1024, 3): 2, (129, 130, 1040, 2): 2, (128, 128, 4099, 0): 8,
             (16, 16, 32768, 0): 64, (16, 16, 32753, 0): 64, (16, 16, 32769, 0): 63, (257, 257, 2049, 0): 4, (1449, 1449, 1025, 0): 2}
TN_EMPTY = [(5, 3, 0, 2), (0, 3, 7, 1), (5, 0, 7, 1)]  # K = 0 with ldc > N: zeros inside; M = 0 and N = 0: nothing touched
TN_CASES = [s + (None,) for s in list(TN_SLICES) + TN_EMPTY] + [(128, 128, 4099, 0, m) for m in ("A", "B")]


def tn_id(c):
    return "%dx%dx%d_pad%d%s" % (c[0], c[1], c[2], c[3], "" if c[4] is None else "_%s_moved" % c[4])


@functools.lru_cache(maxsize=4)
def tn_data(M, N, Kk):
    a, b = ints(17 * M + Kk, (Kk, M)), ints(19 * N + Kk + 1, (Kk, N))
    bounded(np.abs(a).T @ np.abs(b))
    return a, b, RC.exact(a.T @ b + 0.0)


def gemm_tn(ctx, M, N, Kk, pad, moved=None):
    """A (K x M) and B (K x N) at pitches M + pad, N + pad with NaN pad columns, C at pitch N + pad prefilled; the workspace guarded and
    exactly as large as hnh_gemm_tn_f64_workspace says; two runs"""
    lib = ctx.lib
    a, b, prod = tn_data(M, N, Kk)
    lda, ldb, ldc = M + pad, N + pad, N + pad
    need = int(lib.hnh_gemm_tn_f64_workspace(M, N, Kk))
    assert need == tn_workspace(M, N, Kk), (need, tn_workspace(M, N, Kk))
    with Buffers(ctx) as bufs:
        pa, pb = bufs.add("A", padded(a, lda), moved == "A"), bufs.add("B", padded(b, ldb), moved == "B")
        pc = bufs.add("C", np.full((M, ldc), 9.0))
        pw = bufs.add("work", np.full(need, 5.0), scratch=True) if need else None
        want = np.full((M, ldc), 9.0)
        want[:, :N] = prod
        runs = []
        for rnd in range(2):
            c0 = np.full((M, ldc), 9.0 + rnd)
            bufs.a["C"].set(c0)
            want[:, N:] = c0[:, N:]
            ctx.check(lib.hnh_gemm_tn_f64(ctx.h, M, N, Kk, pa, lda, pb, ldb, pc, ldc, pw, need, 0), "gemm_tn")
            runs.append(bufs.verify("gemm_tn %s run %d" % ((M, N, Kk, pad, moved), rnd), C=want)["C"][:, :N])
        assert same_bits(runs[0], runs[1])
        if Kk == 0:
            assert same_bits(runs[0], np.zeros((M, N)))


def gemm_tn_refusals(ctx):
    lib = ctx.lib
    M, N, Kk = 17, 9, 1024
    a, b, _ = tn_data(M, N, Kk)
    need = tn_workspace(M, N, Kk)
    assert need == 2 * M * N
    with Buffers(ctx) as bufs:
        pa, pb, pc = bufs.add("A", a), bufs.add("B", b), bufs.add("C", np.full((M, N), 9.0))
        pw = bufs.add("work", np.full(need, 5.0))
        short = "hnh_gemm_tn_f64: workspace smaller than hnh_gemm_tn_f64_workspace()"
        refused(ctx, lib.hnh_gemm_tn_f64(ctx.h, M, N, Kk, pa, M, pb, N, pc, N, pw, need - 1, 0), short)
        refused(ctx, lib.hnh_gemm_tn_f64(ctx.h, M, N, Kk, pa, M, pb, N, pc, N, None, need, 0), short)
        pitch = "hnh_gemm_tn_f64: leading dimension smaller than the width"
        for lda, ldb, ldc in ((M - 1, N, N), (M, N - 1, N), (M, N, N - 1)):
            refused(ctx, lib.hnh_gemm_tn_f64(ctx.h, M, N, Kk, pa, lda, pb, ldb, pc, ldc, pw, need, 0), pitch)
        bufs.verify("refused gemm_tn calls")


# ------------------------------------------------------------------------------------------------ the row helpers
def lpr_of(chunks, ladder):
    return max(l for l in ladder if l <= max(chunks, 1))


def row_instance(R, aligned, ladder):
    """(LPR, W) of rowdot_kernel (ladder 1 2 4 .. 64) and of cg_step_kernel / row_epilogue_kernel (ladder 1 4 16 64)"""
    w = 2 if (R % 2 == 0 and aligned) else 1
    return lpr_of(R // w, ladder), w


ROWDOT_LADDER, CG_LADDER = (1, 2, 4, 8, 16, 32, 64), (1, 4, 16, 64)
ROWDOT_CASES = [(R, None) for R in (2, 4, 6, 8, 16, 32, 64, 126, 128, 130, 256, 1, 3, 5, 9, 17, 33, 65, 129, 255)] + \
               [(R, m) for m in ("A", "B") for R in (2, 8, 32, 128)]
ROWDOT_EXPECTED = {c: row_instance(c[0], c[1] is None, ROWDOT_LADDER) for c in ROWDOT_CASES}
CG_WIDTHS = [(R, None) for R in (2, 6, 8, 30, 32, 126, 128, 130, 256, 1, 3, 15, 63, 65, 129)]
CG_CASES = CG_WIDTHS + [(R, m) for m in ("X", "Rm", "P", "MP") for R in (4, 16, 128)]
CG_EXPECTED = {c: row_instance(c[0], c[1] is None, CG_LADDER) for c in CG_CASES}
EPILOGUE_CASES = [c + (xs, rd) for c in CG_WIDTHS + [(R, m) for m in ("Out", "X") for R in (4, 16, 128)] for xs in (-0.5, 0.0) for rd in (True, False)]
EPILOGUE_EXPECTED = {c: row_instance(c[0], c[1] is None, CG_LADDER) for c in EPILOGUE_CASES}
SCALE_ADD_CASES = [(R, v, m) for R in (1, 2, 3, 8, 130, 256) for v in ("both", "neither", "yv", "xv") for m in (None,)] + \
                  [(R, "both", m) for R in (1, 2, 3, 8, 130, 256) for m in ("Y", "X")]
SCALE_ADD_PAST = (81921, 256)  # 20 971 776 doubles: the second trip of row_scale_add_kernel<2>
CHUNK_LAYOUTS = [(128, (0, 5, 5, 40, 77)), (7, (0, 3, 30)), (16, (0, 64))]
CHUNK_CASES = [(R, cuts, nb, None) for R, cuts in CHUNK_LAYOUTS for nb in (0, 1, 5)] + \
              [(R, cuts, 5, m) for R, cuts in CHUNK_LAYOUTS if R % 2 == 0 for m in ("dst", "src")]
CHUNK_PAST = (256, (0, 16500), 2, None)  # 2 112 000 pairs in one chunk


def row_id(c):
    return "_".join("R%d" % v if i == 0 else str(v) for i, v in enumerate(c))


def chunk_id(c):
    return "R%d_%dchunks_nb%d%s" % (c[0], len(c[1]) - 1, c[2], "" if c[3] is None else "_%s_moved" % c[3])


def rowdot(ctx, R, moved=None, rows=ROWS):
    a, b = ints(3 * R + 1, (rows, R)), ints(3 * R + 2, (rows, R))
    bounded(np.abs(a * b).sum(axis=1))
    want = RC.exact((a * b).sum(axis=1) + 0.0)
    with Buffers(ctx) as bufs:
        pa, pb, po = bufs.add("A", a, moved == "A"), bufs.add("B", b, moved == "B"), bufs.add("out", np.full(rows, 9.0))
        ctx.check(ctx.lib.hnh_rowdot_f64(ctx.h, pa, pb, po, rows, R, 0), "rowdot")
        bufs.verify("rowdot R=%d moved=%s" % (R, moved), out=want)
    return want


def cg_step_model(x, rm, p, mp, alpha):
    x1, r1 = RC.exact(x + alpha[:, None] * p), RC.exact(rm - alpha[:, None] * mp)
    bounded((r1 * r1).sum(axis=1))
    return x1, r1, RC.exact((r1 * r1).sum(axis=1) + 0.0)


def cg_step(ctx, R, moved=None, rows=ROWS):
    x, rm, p, mp = (ints(5 * R + i, (rows, R)) for i in range(4))
    alpha = pow2(R, rows)
    x1, r1, rs = cg_step_model(x, rm, p, mp, alpha)
    with Buffers(ctx) as bufs:
        ptr = {n: bufs.add(n, h, moved == n) for n, h in (("X", x), ("Rm", rm), ("P", p), ("MP", mp))}
        pal, prs = bufs.add("alpha", alpha), bufs.add("rsnew", np.full(rows, 9.0))
        ctx.check(ctx.lib.hnh_cg_step_f64(ctx.h, ptr["X"], ptr["Rm"], ptr["P"], ptr["MP"], pal, prs, rows, R, 0), "cg_step")
        bufs.verify("cg_step R=%d moved=%s" % (R, moved), X=x1, Rm=r1, rsnew=rs)
    return x1, r1, rs, (x, rm)


def row_epilogue_model(out, x, x_scale):
    out1 = RC.exact(out + x_scale * x) if x_scale != 0.0 else out
    bounded(np.abs(x * out1).sum(axis=1))
    return out1, RC.exact((x * out1).sum(axis=1) + 0.0)


def row_epilogue(ctx, R, moved, x_scale, with_rowdot, rows=ROWS):
    out, x = ints(7 * R + 1, (rows, R)), ints(7 * R + 2, (rows, R))
    out1, dot = row_epilogue_model(out, x, x_scale)
    with Buffers(ctx) as bufs:
        po, px, pd = bufs.add("Out", out, moved == "Out"), bufs.add("X", x, moved == "X"), bufs.add("rowdot", np.full(rows, 9.0))
        ctx.check(ctx.lib.hnh_row_epilogue_f64(ctx.h, po, px, x_scale, pd if with_rowdot else None, rows, R, 0), "row_epilogue")
        outs = dict(Out=out1)  # (x_scale = 0: out1 IS the uploaded array, so Out must come back bit-identical)
        if with_rowdot:
            outs["rowdot"] = dot
        bufs.verify("row_epilogue R=%d moved=%s x_scale=%s rowdot=%s" % (R, moved, x_scale, with_rowdot), **outs)
    return out, out1, dot


def row_scale_add(ctx, R, vectors="both", moved=None, rows=ROWS):
    """Y = ya yv Y + xa xv X with ya = 0.5, xa = -1; Y has no zero, so that no term pair can add up to a negative zero"""
    y, x = ints(9 * R + 1, (rows, R), zeros=0.0), ints(9 * R + 2, (rows, R))
    yv, xv = pow2(R + 1, rows), pow2(R + 2, rows)
    use_y, use_x = vectors in ("both", "yv"), vectors in ("both", "xv")
    ya, xa = 0.5, -1.0
    fy, fx = ya * (yv if use_y else np.ones(rows)), xa * (xv if use_x else np.ones(rows))
    ty, tx = fy[:, None] * y, fx[:, None] * x  # (tx may hold -0.0; ty never is a zero, so no result is a negative one)
    bounded(np.abs(ty) + np.abs(tx))
    want = RC.exact(ty + tx)
    with Buffers(ctx) as bufs:
        py, px = bufs.add("Y", y, moved == "Y"), bufs.add("X", x, moved == "X")
        pyv, pxv = bufs.add("yv", yv), bufs.add("xv", xv)
        ctx.check(ctx.lib.hnh_row_scale_add_f64(ctx.h, py, pyv if use_y else None, ya, px, pxv if use_x else None, xa, rows, R, 0), "row_scale_add")
        bufs.verify("row_scale_add R=%d %s moved=%s rows=%d" % (R, vectors, moved, rows), Y=want)
    return y, want


def sum_chunked_model(dst0, src, cuts, nb, q0, q1):
    want = dst0.copy()
    for q in range(q0, q1):
        w = cuts[q + 1] - cuts[q]
        for k in range(nb):  # block order (any order gives these bits)
            want[cuts[q]:cuts[q + 1]] += src[nb * cuts[q] + k * w: nb * cuts[q] + (k + 1) * w]
    return RC.exact(want)


def sum_chunked(ctx, R, cuts, nb, moved=None):
    """every window (q0, q1) of the existing test over one layout"""
    rows, nch = cuts[-1], len(cuts) - 1
    dst0, src = ints(R + nb, (rows, R)), ints(R + nb + 1, (nb * rows, R))
    ch = np.array(cuts, dtype=np.int64)
    with Buffers(ctx) as bufs:
        pd, ps = bufs.add("dst", dst0, moved == "dst"), bufs.add("src", src, moved == "src")
        for q0, q1 in sorted({(0, nch), (min(1, nch), nch), (0, 1)}):
            bufs.a["dst"].set(dst0)
            ctx.check(ctx.lib.hnh_sum_chunked_blocks_f64(ctx.h, pd, ps, nb, nch, ch.ctypes.data_as(C.c_void_p), q0, q1, R, 0), "sum_chunked")
            bufs.verify("sum_chunked R=%d cuts=%s nb=%d moved=%s [%d, %d)" % (R, cuts, nb, moved, q0, q1), dst=sum_chunked_model(dst0, src, cuts, nb, q0, q1))


# ------------------------------------------------------------------------------------------------ the element-wise kernels
ALPHA = 0.25


def leaky(v):
    return RC.exact(np.where(v > 0, v, ALPHA * v))


class Ew:
    """one element-wise kernel: build(shape) -> (operands name -> host array in argument order, call(lib, h, ptr), outputs name -> model)"""

    def __init__(self, build, operands, grad=False, cols=False, unrolled=False):
        self.build, self.operands, self.grad, self.cols, self.unrolled = build, operands, grad, cols, unrolled

    def shape(self, n):
        return COLS_SHAPE[n] if self.cols else n

    def past_cap(self):
        return PAST_COLS if self.cols else (PAST_UNROLLED if self.unrolled else PAST_PLAIN)


def _leaky_relu(n):
    v = ints(1, n)
    return dict(v=v), lambda lib, h, p: lib.hnh_leaky_relu_f64(h, p["v"], ALPHA, n, 0), dict(v=leaky(v))


def _leaky_relu_grad(n):
    e, d = ints(2, n, zeros=0.1), ints(3, n)
    return dict(e=e, d=d), lambda lib, h, p: lib.hnh_leaky_relu_grad_f64(h, p["e"], p["d"], ALPHA, n, 0), \
        dict(e=leaky(e), d=RC.exact(np.where(e > 0, d, d * ALPHA)))


def _relu_store_cols(shape):
    rows, cols = shape
    col0, ld = 2, cols + 5
    src, dst = ints(4, (rows, cols), zeros=0.1), ints(5, (rows, ld))
    want = dst.copy()
    want[:, col0:col0 + cols] = np.maximum(src, 0.0)
    return dict(dst=dst, src=src), lambda lib, h, p: lib.hnh_relu_store_cols_f64(h, p["dst"], ld, col0, p["src"], rows, cols, 0), dict(dst=RC.exact(want))


def _relu_grad_cols(shape):
    rows, cols = shape
    col0, ld_dz, ld_g, ld_out = 2, cols + 3, cols + 5, cols + 3
    g, out, dz = padded(ints(6, (rows, col0 + cols)), ld_g), padded(ints(7, (rows, col0 + cols), zeros=0.1), ld_out), ints(8, (rows, ld_dz))
    want = dz.copy()
    want[:, :cols] = np.where(out[:, col0:col0 + cols] > 0, g[:, col0:col0 + cols], 0.0)
    return dict(dZ=dz, G=g, out=out), lambda lib, h, p: lib.hnh_relu_grad_cols_f64(h, p["dZ"], ld_dz, p["G"], ld_g, p["out"], ld_out, col0, rows, cols, 0), \
        dict(dZ=RC.exact(want))


def _sum3_cols(shape):
    rows, cols = shape
    col0, ld = 2, cols + 5
    x, y, z, dst = ints(9, (rows, cols)), ints(10, (rows, cols)), ints(11, (rows, cols)), ints(12, (rows, ld))
    want = dst.copy()
    want[:, col0:col0 + cols] = (x + y) + z + 0.0
    return dict(dst=dst, x=x, y=y, z=z), lambda lib, h, p: lib.hnh_sum3_cols_f64(h, p["dst"], ld, col0, p["x"], p["y"], p["z"], rows, cols, 0), \
        dict(dst=RC.exact(want))


def _transpose_into(shape):
    rows, cols = shape
    row0, ld = 1, rows + 3
    w, dst = ints(13, (rows, cols)), ints(14, (row0 + cols + 1, ld))
    want = dst.copy()
    want[row0:row0 + cols, :rows] = w.T
    return dict(dst=dst, W=w), lambda lib, h, p: lib.hnh_transpose_into_f64(h, p["dst"], ld, row0, p["W"], rows, cols, 0), dict(dst=want)


HASH_SEED, HASH_SCALE = 42, 0.5


def _fill_hashed(shape):
    """bit for bit oracle.hashed_uniform (times a power of two) of the global keys of a block at (5, 3) of a matrix cols + 7 wide"""
    rows, cols = shape
    top, left, rg = 5, 3, cols + 7
    keys = (top + np.arange(rows, dtype=np.uint64))[:, None] * np.uint64(rg) + np.uint64(left) + np.arange(cols, dtype=np.uint64)[None, :]
    want = O.hashed_uniform(keys.reshape(-1), HASH_SEED) * HASH_SCALE
    return dict(dst=np.full(rows * cols, 9.0)), lambda lib, h, p: lib.hnh_fill_hashed_f64(h, p["dst"], rows, cols, top, left, rg, HASH_SEED, HASH_SCALE, 0), \
        dict(dst=want)


def _vec_add_scalar(n):
    v = ints(15, n)
    return dict(v=v), lambda lib, h, p: lib.hnh_vec_add_scalar_f64(h, p["v"], 0.25, n, 0), dict(v=RC.exact(v + 0.25))


def _vec_div(n):
    num = ints(16, n, zeros=0.0)
    den = np.resize(np.concatenate([POW2, [4.0, -4.0]]), n)
    return dict(out=np.full(n, 9.0), num=num, den=den), lambda lib, h, p: lib.hnh_vec_div_f64(h, p["out"], p["num"], p["den"], n, 0), \
        dict(out=RC.exact(num / den))


def _fill(value):
    def build(n):
        return dict(dst=ints(17, n)), lambda lib, h, p: lib.hnh_fill_f64(h, p["dst"], n, value, 0), dict(dst=np.full(n, value))
    return build


def _hadamard(alias):
    def build(n):
        a, b = ints(18, n, zeros=0.0), ints(19, n, zeros=0.0)
        want = RC.exact(a * b)
        if alias is None:
            return dict(out=np.full(n, 9.0), a=a, b=b), lambda lib, h, p: lib.hnh_hadamard_f64(h, p["out"], p["a"], p["b"], n, 0), dict(out=want)
        if alias == "a":
            return dict(a=a, b=b), lambda lib, h, p: lib.hnh_hadamard_f64(h, p["a"], p["a"], p["b"], n, 0), dict(a=want)
        return dict(a=a, b=b), lambda lib, h, p: lib.hnh_hadamard_f64(h, p["b"], p["a"], p["b"], n, 0), dict(b=want)
    return build


def _axpy(n):
    y, x = ints(20, n), ints(21, n)
    return dict(y=y, x=x), lambda lib, h, p: lib.hnh_axpy_f64(h, p["y"], p["x"], -0.5, n, 0), dict(y=RC.exact(y + -0.5 * x))


EW = {
    "leaky_relu": Ew(_leaky_relu, ("v",)),
    "leaky_relu_grad": Ew(_leaky_relu_grad, ("e", "d"), grad=True),
    "relu_store_cols": Ew(_relu_store_cols, ("dst", "src"), cols=True),
    "relu_grad_cols": Ew(_relu_grad_cols, ("dZ", "G", "out"), grad=True, cols=True),
    "sum3_cols": Ew(_sum3_cols, ("dst", "x", "y", "z"), grad=True, cols=True),
    "transpose_into": Ew(_transpose_into, ("dst", "W"), grad=True, cols=True),
    "fill_hashed": Ew(_fill_hashed, ("dst",), cols=True),
    "vec_add_scalar": Ew(_vec_add_scalar, ("v",)),
    "vec_div": Ew(_vec_div, ("out", "num", "den")),
    "fill_2.5": Ew(_fill(2.5), ("dst",), unrolled=True),
    "fill_0": Ew(_fill(0.0), ("dst",), unrolled=True),
    "hadamard": Ew(_hadamard(None), ("out", "a", "b"), unrolled=True),
    "hadamard_out_is_a": Ew(_hadamard("a"), ("a", "b"), unrolled=True),
    "hadamard_out_is_b": Ew(_hadamard("b"), ("a", "b"), unrolled=True),
    "axpy": Ew(_axpy, ("y", "x"), unrolled=True),
}
EW_CASES = [(name, m) for name, e in EW.items() for m in (None,) + e.operands]
# the kernels that run once past their cap (the in-place Hadamard and the memset path of fill run the same loop or none)
EW_PAST = [n for n in EW if n not in ("fill_0", "hadamard_out_is_a", "hadamard_out_is_b")]


def ew_id(c):
    return c[0] + ("" if c[1] is None else "_%s_moved" % c[1])


def run_ew(ctx, name, shape, moved=None):
    e = EW[name]
    operands, call, outputs = e.build(shape)
    assert tuple(operands) == e.operands
    with Buffers(ctx) as bufs:
        ptr = {n: bufs.add(n, h, moved == n) for n, h in operands.items()}
        ctx.check(call(ctx.lib, ctx.h, ptr), name)
        bufs.verify("%s %s moved=%s" % (name, shape, moved), **outputs)
    return operands, outputs


def run_ew_sizes(ctx, name, moved=None):
    for n in EW_SIZES:
        run_ew(ctx, name, EW[name].shape(n), moved)


# hnh_fill_f64(-0.0) is NOT among the cases: the device takes the memset path (-0.0 == 0.0) and writes +0.0, the double writes -0.0.
# DESIGN.md §6e says why that difference is left open.
