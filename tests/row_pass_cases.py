"""What tests/test_row_instances_cpu.py and tests/test_row_instances_gpu.py share (not itself a test): the graphs, the integer data, the
numpy model, the guarded device buffers and the calls of the three row passes of include/hnh_kernels.h (SDDMM, SpMM, fused SDDMM+SpMM),
and the table of kernel instances each (operation, width, alignment, switches) is expected to launch.

EXACT ARITHMETIC.  Every input is a small integer (X, Y in [-4, 4]; values, Out in [-8, 8]) or a power of two times one (svalues in
{-2, -1, -0.5, 0.5, 1, 2}, LeakyReLU alpha 0.25, x_scale -0.5), so every product and every partial sum is a multiple of 2^-4 far below
2^53: any order of addition (FMA or not, a butterfly, hub-row segments, hardware atomics) gives the same bits, and the tests compare bit
patterns, not distances.  The model asserts that precondition on the sums of absolute values (exact(), bounded()), which bound every
partial sum in every order.  Signed zeros: the kernels start every sum from +0.0, so does the model (`+ 0.0`); the sign of a zero
RESULT is the one thing that depends on how a sum is split, so the data keep every result clear of -0.0 (Data) and exact() asserts it.

GUARDED BUFFERS.  Every device array (operands too) lies between two guards of 128 bytes filled with one quiet-NaN bit pattern; the
pointer handed to the library is the interior (128-byte aligned like the allocation), optionally moved by one element.  After every call
the guards of all arrays must hold the pattern, the inputs must be what was uploaded and the outputs what the model says.  The guards are
as long as the longest stray READ the line-granular NARROW instances make by design (one line of `values`, one 32-index block of
`colidx`, masked before use): a NaN that leaks from there into a result is caught like any wrong number."""
import ctypes as C
import functools

import numpy as np

from distributed_sddmm_amd import _kernels as K

EDGE = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65]  # row lengths round the unroll batches (8, half 4) and the 16-nonzero trips
GUARD_BYTES = 128
PATTERN = np.uint64(0x7FF8C0DEC0DEC0DE)  # a quiet NaN; as int32 pairs: one negative, one huge index
ALPHA, X_SCALE = 0.25, -0.5
SVALUES = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
VOW, OOW, LEAKY = K.FUSED_VALUES_OVERWRITE, K.FUSED_OUT_OVERWRITE, K.FUSED_LEAKY_RELU
ALIGNMENTS = ("a16", "dense8", "csr1")  # all 16-byte aligned / X, Y, Out moved by 8 bytes / values, svalues and colidx moved by one element

# the widths of the GPU file, by the path they take when every dense operand is 16-byte aligned
W_EXACT = [2, 4, 8, 16, 32, 64, 128, 192, 256, 320, 384, 448, 512]
W_NX2 = [6, 100, 126, 130, 254, 258, 510]
W_TILES2 = [514, 600]
W_ODD = [1, 3, 63, 65, 127, 129, 255, 257, 301]
W_DENSE8 = [64, 128, 256, 384]  # every dense operand moved by 8 bytes: W = 1 at even widths
W_CSR1 = [8, 16, 32]            # values / svalues / colidx moved by one element: the plain instances instead of NARROW
WIDTH_CASES = [(w, "a16") for w in W_EXACT + W_NX2 + W_TILES2 + W_ODD] + [(w, "dense8") for w in W_DENSE8] + [(w, "csr1") for w in W_CSR1]
W_SWITCHES = [2, 16, 64, 100, 128, 256, 300, 448, 600, 3, 129, 301]  # one per instance family, for the context switches
W_WINDOWS = [16, 100, 128, 257, 600]


def case_id(p):
    return "R%d_%s" % p


# ------------------------------------------------------------------------------------------------ graphs
class Graph:
    def __init__(self, rowptr, colidx, cols):
        self.rowptr, self.colidx, self.cols = np.asarray(rowptr, np.int32), np.asarray(colidx, np.int32), int(cols)
        self.rows, self.nnz = len(self.rowptr) - 1, len(self.colidx)
        self.lens = np.diff(self.rowptr)
        self.ridx = np.repeat(np.arange(self.rows, dtype=np.int32), self.lens)
        self.max_row = int(self.lens.max()) if self.rows else 0
        assert self.rowptr[0] == 0 and self.rowptr[-1] == self.nnz and np.all(self.lens >= 0)
        for r in range(self.rows):  # sorted and distinct within a row, inside the block
            c = self.colidx[self.rowptr[r]:self.rowptr[r + 1]]
            assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 0 and c[-1] < cols))


def _from_lens(lens, cols, seed, ends_in):
    """rows of the given lengths with sorted distinct columns; row `ends_in` holds column 0 and column cols - 1"""
    rng = np.random.default_rng(seed)
    parts = []
    for r, n in enumerate(lens):
        if r == ends_in:
            assert n >= 2
            c = np.concatenate([[0], 1 + np.sort(rng.choice(cols - 2, n - 2, replace=False)), [cols - 1]])
        else:
            c = np.sort(rng.choice(cols, n, replace=False))
        parts.append(c)
    colidx = np.concatenate(parts) if parts else np.zeros(0)
    return Graph(np.concatenate([[0], np.cumsum(lens)]), colidx, cols)


@functools.lru_cache(maxsize=None)
def edge_graph(rows=523, cols=300, tail_empty=False):
    """Row i has EDGE[i % 15] nonzeros: row 0 is empty, the last row is not (tail_empty: the last 3 rows are).  523 is prime and above
    2 x 256, so no instance's rows per workgroup (1 .. 256) divides it and every instance runs more than two workgroups."""
    lens = np.array([EDGE[i % len(EDGE)] for i in range(rows)])
    if tail_empty:
        lens[-3:] = 0
    g = _from_lens(lens, cols, 7 + tail_empty, ends_in=14)
    assert g.lens[0] == 0 and (g.lens[-1] > 0) != tail_empty and g.colidx.min() == 0 and g.colidx.max() == cols - 1
    return g


HUB_LENS = {42: 64, 45: 65, 50: 256, 55: 257, 60: 512, 65: 513, 69: 700}  # (rows whose background lengths 0 .. 40 occur elsewhere too)


@functools.lru_cache(maxsize=None)
def hub_graph():
    """70 x 1024, background rows of 0 .. 40 nonzeros and rows of 64 (stays in the row kernel under HNH_LONG_ROW=64), 65, 256 (one
    segment of 256), 257, 512 (two), 513 and 700 (three; the last row of the block)."""
    lens = np.array([i % 41 for i in range(70)])
    for r, n in HUB_LENS.items():
        lens[r] = n
    return _from_lens(lens, 1024, 11, ends_in=69)


@functools.lru_cache(maxsize=None)
def degenerate_graph(kind):
    if kind == "all_empty":
        return Graph(np.zeros(71, np.int32), np.zeros(0, np.int32), 300)
    if kind == "one_row":
        return _from_lens(np.array([17]), 300, 3, ends_in=0)
    assert kind == "one_row_one_nonzero"
    return Graph(np.array([0, 1]), np.array([299]), 300)


# ------------------------------------------------------------------------------------------------ integer data
def _ints(rng, k, shape, zeros=0.03):
    """integers of [-k, k]; few zeros, so that products and sums rarely vanish (the shares are asserted in the CPU file)"""
    v = rng.integers(1, k + 1, shape) * rng.choice([-1, 1], shape)
    v[rng.random(shape) < zeros] = 0
    return v.astype(np.float64)


class Data:
    def __init__(self, g, R, seed=0):
        rng = np.random.default_rng(1000 * R + g.rows + seed)
        self.R = R
        self.X, self.Y = _ints(rng, 4, (g.rows, R)), _ints(rng, 4, (g.cols, R))
        self.v0, self.out0 = _ints(rng, 8, g.nnz), _ints(rng, 8, (g.rows, R))  # the state to accumulate onto, garbage for the overwrite flags
        self.sv = rng.choice(SVALUES, g.nnz)
        # No result may be a NEGATIVE zero: its sign is the one thing that does depend on how a sum is split (s d1 + s d2 = +0.0 but
        # s (d1 + d2) = -0.0 for d1 = -d2, s < 0: column slabs and tiles against one pass) and is no error.  A zero times a negative
        # svalue is the only source of one here, so a nonzero whose dot product or updated value vanishes gets a positive svalue.
        d = (self.X[g.ridx] * self.Y[g.colidx]).sum(axis=1)
        zero = (d == 0) | (self.v0 + d == 0)
        self.sv[zero] = np.abs(self.sv[zero])


@functools.lru_cache(maxsize=None)
def data_for(g, R):
    return Data(g, R)


# ------------------------------------------------------------------------------------------------ the numpy model
def exact(*arrays):
    """the precondition of bit equality: multiples of 2^-4 below 2^40, no negative zero"""
    for a in arrays:
        a = np.asarray(a)
        assert np.all(a * 16 == np.rint(a * 16)) and (a.size == 0 or np.max(np.abs(a)) < 2.0 ** 40), "inputs leave the exact range"
        assert not np.any(np.signbit(a) & (a == 0)), "a negative zero: its sign depends on how the sum is split"
    return arrays[0]


def _row_sums(g, terms):
    """sum of the nonzeros' terms (nnz x R) per row -> rows x R, started from +0.0"""
    out = np.zeros((g.rows, terms.shape[1]))
    live = g.lens > 0
    if g.nnz:
        out[live] += np.add.reduceat(terms, g.rowptr[:-1][live], axis=0)
    return out


def dots(g, X, Y):
    p = X[g.ridx] * Y[g.colidx]
    exact(np.abs(p).sum(axis=1))  # bounds every partial sum in every order
    return exact(p.sum(axis=1) + 0.0)


def sddmm(g, v0, X, Y, scale=None, overwrite=False):
    """values (+)= scale . <X_r, Y_c> (sparse_kernels.cpp:44-55, with the closing Hadamard of hnh_sddmm_csr_ps)"""
    d = dots(g, X, Y)
    if scale is not None:
        d = exact(scale * d)
    return d if overwrite else exact(v0 + d)


def spmm(g, w, Y, out0, overwrite=False):
    """Out (+)= S Y (sparse_kernels.cpp:95-107, beta = 1)"""
    t = w[:, None] * Y[g.colidx]
    base = np.zeros_like(out0) if overwrite else out0
    exact(np.abs(base) + _row_sums(g, np.abs(t)))
    return exact(base + _row_sums(g, t))


def fused(g, v0, sv, X, Y, out0, flags, alpha=0.0, x_scale=0.0, rowdot=False):
    """hnh_fused_sddmm_spmm_csr_x: values (+)= dots; with LEAKY_RELU the stored value is LeakyReLU(svalues . values) and weighs the SpMM
    half, without it values . svalues does; then Out += x_scale X and rowdot = <X, Out> -> (values, Out, rowdot or None)"""
    vals = sddmm(g, v0, X, Y, overwrite=bool(flags & VOW))
    if flags & LEAKY:
        if sv is not None:
            vals = exact(vals * sv)
        vals = exact(np.where(vals > 0, vals, alpha * vals))
        w = vals
    else:
        w = vals if sv is None else exact(vals * sv)
    out = spmm(g, w, Y, out0, overwrite=bool(flags & OOW))
    if x_scale != 0.0:
        out = exact(out + x_scale * X)
    dot = None
    if rowdot:
        exact(np.abs(X * out).sum(axis=1))
        dot = exact((X * out).sum(axis=1) + 0.0)
    return vals, out, dot


def window_splits(g, bounds):
    """hnh_csr_window_bounds: split[b, r] = first nonzero of row r with column >= bounds[b]"""
    s = np.zeros((len(bounds), g.rows), np.int32)
    for r in range(g.rows):
        lo, hi = g.rowptr[r], g.rowptr[r + 1]
        s[:, r] = lo + np.searchsorted(g.colidx[lo:hi], bounds, side="left")
    return s


# ------------------------------------------------------------------------------------------------ contexts
class DoubleCtx(K.Ctx):
    """the oracle's C test double behind the same ABI (oracle/hnh_oracle_backend.c): a context of it with K.Ctx's helpers"""

    def __init__(self, path):
        self.lib = K.load(path)
        assert self.lib.hnh_backend_name() == b"oracle-cpu-test-double"
        h = C.c_void_p()
        assert self.lib.hnh_ctx_create(0, C.byref(h)) == K.OK
        self.h = h


# ------------------------------------------------------------------------------------------------ guarded device buffers
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class Guarded:
    """One device array between two guards.  `shift` elements of guard more in front move the interior off its 128-byte alignment."""

    def __init__(self, ctx, host, shift=0, name=""):
        self.ctx, self.name = ctx, name
        host = np.ascontiguousarray(host)
        self.shape, self.dtype, item = host.shape, host.dtype, host.dtype.itemsize
        assert item in (4, 8) and GUARD_BYTES % item == 0
        self.lo = GUARD_BYTES + shift * item
        self.hi = self.lo + host.nbytes
        self.nbytes = (self.hi + GUARD_BYTES + 7) // 8 * 8  # at least 128 bytes behind, whole uint64 words
        self.base = ctx.alloc(self.nbytes)
        assert self.base % 128 == 0, "hnh_malloc must return 128-byte aligned memory (the NARROW instances depend on it)"
        self.ptr = self.base + self.lo
        self.blank = np.full(self.nbytes // 8, PATTERN, np.uint64)
        self.set(host)

    def set(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.shape == self.shape
        self.host = host.copy()
        img = self.blank.copy()
        img.view(np.uint8)[self.lo:self.hi] = host.reshape(-1).view(np.uint8)
        self.ctx.check(self.ctx.lib.hnh_memcpy(self.ctx.h, self.base, img.ctypes.data, self.nbytes, K.H2D, K.STREAM_COMPUTE), "h2d")
        self.ctx.sync()

    def fetch(self):
        """(the interior, whether both guards hold the pattern: compared as uint64 words with the interior blanked)"""
        img = np.empty(self.nbytes // 8, np.uint64)
        self.ctx.sync()
        self.ctx.check(self.ctx.lib.hnh_memcpy(self.ctx.h, img.ctypes.data, self.base, self.nbytes, K.D2H, K.STREAM_COMPUTE), "d2h")
        self.ctx.sync()
        inner = img.view(np.uint8)[self.lo:self.hi].copy().view(self.dtype).reshape(self.shape)
        img.view(np.uint8)[self.lo:self.hi] = self.blank.view(np.uint8)[self.lo:self.hi]
        return inner, bool(np.array_equal(img, self.blank))

    def free(self):
        if self.base:
            self.ctx.free(self.base)
            self.base = None


def describe(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    i = tuple(bad[0])
    return "%d of %d entries differ, first at %s: got %r, model %r" % (len(bad), got.size, i, got[i], want[i])


class Block:
    """The device arrays of one (graph, data, alignment class) and the calls on them.  Every call resets the outputs it needs, runs,
    and verify()s: the guards of ALL arrays, the inputs bit for bit, the outputs against the model."""

    INPUTS = ("rowptr", "colidx", "ridx", "X", "Y", "sv")

    def __init__(self, ctx, g, d, align="a16"):
        assert align in ALIGNMENTS
        self.ctx, self.lib, self.g, self.d, self.R, self.align = ctx, ctx.lib, g, d, d.R, align
        dense, csr = int(align == "dense8"), int(align == "csr1")
        mk = lambda name, a, shift: Guarded(ctx, a, shift, name)  # noqa: E731
        self.a = dict(rowptr=mk("rowptr", g.rowptr, 0), colidx=mk("colidx", g.colidx, csr), ridx=mk("ridx", g.ridx, 0),
                      X=mk("X", d.X, dense), Y=mk("Y", d.Y, dense), sv=mk("svalues", d.sv, csr), values=mk("values", d.v0, csr),
                      out=mk("Out", d.out0, dense), rowdot=mk("rowdot", np.full(g.rows, 9.0), 0))
        for n in ("X", "Y", "out"):
            assert self.a[n].ptr % 16 == (8 if dense else 0)
        for n in ("colidx", "values", "sv"):
            assert (self.a[n].ptr % 128 == 0) == (not csr)
        self.plan = None

    def p(self, name):
        return self.a[name].ptr

    def free(self):
        if self.plan is not None:
            self.ctx.check(self.lib.hnh_csr_plan_destroy(self.ctx.h, self.plan), "plan destroy")
            self.plan = None
        for a in self.a.values():
            a.free()

    def reset(self, values=None, out=None):
        self.a["values"].set(self.d.v0 if values is None else values)
        self.a["out"].set(self.d.out0 if out is None else out)
        self.a["rowdot"].set(np.full(self.g.rows, 9.0))

    def verify(self, what, **outputs):
        """outputs: name -> the model's array; every other array must be what was uploaded"""
        self.ctx.sync()
        for name, arr in self.a.items():
            got, guards = arr.fetch()
            assert guards, "%s: a guard of %s was overwritten" % (what, arr.name)
            want = outputs.get(name, arr.host)
            want = np.ascontiguousarray(want, dtype=arr.dtype)
            kind = "output" if name in outputs else ("input" if name in self.INPUTS else "untouched buffer")
            assert same_bits(got, want), "%s: %s %s: %s" % (what, kind, arr.name, describe(got, want))

    def hints(self, hinted):
        g = self.g
        return (g.nnz, g.max_row, g.cols) if hinted else (-1, -1, -1)

    def block(self, with_plan=False):
        g = self.g
        if with_plan and self.plan is None:
            self.plan = C.c_void_p()
            self.ctx.check(self.lib.hnh_csr_plan_create(self.ctx.h, C.byref(self.plan)), "plan")
        return K.CsrBlock(g.rows, g.nnz, g.cols, g.max_row, 0, self.p("rowptr"), self.p("colidx"), self.plan if with_plan else None)

    # ---- SDDMM
    def sddmm_ex(self, hinted):
        g, d, c = self.g, self.d, self.ctx
        self.reset()
        c.check(self.lib.hnh_sddmm_csr_ex(c.h, g.rows, self.p("rowptr"), self.p("colidx"), self.p("values"), self.p("X"), self.p("Y"), self.R,
                                          *self.hints(hinted), 0), "sddmm_csr_ex")
        self.verify("sddmm_csr_ex hinted=%s" % hinted, values=sddmm(g, d.v0, d.X, d.Y))

    def sddmm_coo(self):
        g, d, c = self.g, self.d, self.ctx
        self.reset()
        c.check(self.lib.hnh_sddmm_coo(c.h, g.nnz, self.p("ridx"), self.p("colidx"), self.p("values"), self.p("X"), self.p("Y"), self.R, 0), "sddmm_coo")
        self.verify("sddmm_coo", values=sddmm(g, d.v0, d.X, d.Y))

    def sddmm_p(self, scaled, overwrite, with_plan=False, tag=""):
        g, d, c = self.g, self.d, self.ctx
        self.reset()
        blk = self.block(with_plan)
        c.check(self.lib.hnh_sddmm_csr_ps(c.h, C.byref(blk), self.p("values"), self.p("sv") if scaled else None, self.p("X"), self.p("Y"), self.R,
                                          VOW if overwrite else 0, None, 0), "sddmm_csr_ps")
        self.verify("sddmm_csr_ps scaled=%s overwrite=%s %s" % (scaled, overwrite, tag),
                    values=sddmm(g, d.v0, d.X, d.Y, d.sv if scaled else None, overwrite))

    # ---- SpMM
    def spmm_ex(self, hinted):
        g, d, c = self.g, self.d, self.ctx
        self.reset()
        c.check(self.lib.hnh_spmm_csr_ex(c.h, g.rows, self.p("rowptr"), self.p("colidx"), self.p("values"), self.p("Y"), self.p("out"), self.R,
                                         *self.hints(hinted), 0), "spmm_csr_ex")
        self.verify("spmm_csr_ex hinted=%s" % hinted, out=spmm(g, d.v0, d.Y, d.out0))

    def spmm_p(self, overwrite, with_plan=False, tag=""):
        g, d, c = self.g, self.d, self.ctx
        self.reset()
        blk = self.block(with_plan)
        c.check(self.lib.hnh_spmm_csr_pf(c.h, C.byref(blk), self.p("values"), self.p("Y"), self.p("out"), self.R, OOW if overwrite else 0, None, 0),
                "spmm_csr_pf")
        self.verify("spmm_csr_pf overwrite=%s %s" % (overwrite, tag), out=spmm(g, d.v0, d.Y, d.out0, overwrite))

    # ---- fused
    def fused_x(self, flags, use_sv, epilogue=False, hinted=True, via="x", tag=""):
        """via: "x" = hnh_fused_sddmm_spmm_csr_x, "p" / "plan" = hnh_fused_sddmm_spmm_csr_p without / with a structure plan"""
        g, d, c = self.g, self.d, self.ctx
        self.reset()
        ex = K.FusedExtras(ALPHA, X_SCALE if epilogue else 0.0, self.p("rowdot") if epilogue else None, None, None, 0)
        pex = C.byref(ex) if (epilogue or flags & LEAKY) else None
        sv = self.p("sv") if use_sv else None
        if via == "x":
            rc = self.lib.hnh_fused_sddmm_spmm_csr_x(c.h, g.rows, self.p("rowptr"), self.p("colidx"), self.p("values"), sv, self.p("X"), self.p("Y"),
                                                     self.p("out"), self.R, flags, *self.hints(hinted), pex, 0)
        else:
            blk = self.block(via == "plan")
            rc = self.lib.hnh_fused_sddmm_spmm_csr_p(c.h, C.byref(blk), self.p("values"), sv, self.p("X"), self.p("Y"), self.p("out"), self.R, flags, pex,
                                                     None, 0)
        what = "fused_%s flags=%d svalues=%s epilogue=%s hinted=%s %s" % (via, flags, use_sv, epilogue, hinted, tag)
        c.check(rc, what)
        vals, out, dot = fused(g, d.v0, d.sv if use_sv else None, d.X, d.Y, d.out0, flags, ALPHA, X_SCALE if epilogue else 0.0, epilogue)
        outs = dict(values=vals, out=out)
        if epilogue:
            outs["rowdot"] = dot
        self.verify(what, **outs)

    # ---- the operations of one width
    def every_operation(self):
        for hinted in (True, False):
            self.sddmm_ex(hinted)
        self.sddmm_coo()
        for overwrite in (False, True):
            self.sddmm_p(True, overwrite)
        self.spmm_ex(True)
        self.spmm_p(True)
        for flags in (0, VOW, OOW, VOW | OOW):
            for use_sv in (False, True):
                for leaky in (0, LEAKY):
                    self.fused_x(flags | leaky, use_sv)
        self.fused_x(VOW | OOW | LEAKY, True, epilogue=True)
        self.fused_x(0, False, epilogue=True, hinted=False)

    def switch_operations(self):
        """the calls a context switch (panels, slabs, NARROW off, hub rows) is checked with: fewer flag combinations, every kernel family"""
        for hinted in (True, False):
            self.sddmm_ex(hinted)
            self.spmm_ex(hinted)
        self.sddmm_p(True, True)
        self.spmm_p(True)
        for flags, use_sv, epi in ((0, False, False), (VOW | OOW, True, False), (VOW | OOW | LEAKY, True, True), (LEAKY, False, False), (0, True, True)):
            self.fused_x(flags, use_sv, epilogue=epi)
        self.fused_x(VOW | OOW | LEAKY, False, epilogue=True, hinted=False)

    def planned_operations(self):
        """through a block descriptor with a structure plan, twice: the second round reuses the plan's cached hub list and panel splits"""
        for rnd in range(2):
            tag = "planned round %d" % rnd
            self.sddmm_p(False, False, with_plan=True, tag=tag)
            self.sddmm_p(True, True, with_plan=True, tag=tag)
            self.spmm_p(False, with_plan=True, tag=tag)
            self.spmm_p(True, with_plan=True, tag=tag)
            self.fused_x(VOW | OOW | LEAKY, True, epilogue=True, via="plan", tag=tag)
            self.fused_x(0, False, via="plan", tag=tag)

    # ---- windows
    def windows(self, bounds):
        """hnh_csr_window_bounds, then every pass window by window: the result of the whole block, bit for bit"""
        g, d, c, lib = self.g, self.d, self.ctx, self.lib
        bounds = np.asarray(bounds, np.int32)
        nb, nw = len(bounds), len(bounds) + 1
        split = Guarded(c, np.full((nb, g.rows), -7, np.int32), 0, "window splits")
        self.a["split"] = split
        try:
            c.check(lib.hnh_csr_window_bounds(c.h, g.rows, self.p("rowptr"), self.p("colidx"), nb, bounds.ctypes.data_as(C.c_void_p), split.ptr, 0), "bounds")
            want_split = window_splits(g, bounds)
            self.verify("window bounds", split=want_split)
            split.host = want_split  # an input from here on
            assert any(np.array_equal(want_split[q], want_split[q - 1]) for q in range(1, nb)), "one window must be empty"

            def window(q):
                beg = None if q == 0 else split.ptr + (q - 1) * g.rows * 4
                end = None if q == nw - 1 else split.ptr + q * g.rows * 4
                return K.CsrWindow(beg, end, 1 if q == nw - 1 else 0)

            self.reset()
            for q in range(nw):
                c.check(lib.hnh_sddmm_csr_w(c.h, g.rows, self.p("rowptr"), self.p("colidx"), self.p("values"), self.p("X"), self.p("Y"), self.R, g.nnz,
                                            g.max_row, C.byref(window(q)), 0), "sddmm_w")
            self.verify("sddmm_csr_w", values=sddmm(g, d.v0, d.X, d.Y))
            self.reset()
            for q in range(nw):
                c.check(lib.hnh_spmm_csr_w(c.h, g.rows, self.p("rowptr"), self.p("colidx"), self.p("values"), self.p("Y"), self.p("out"), self.R, g.nnz,
                                           g.max_row, C.byref(window(q)), 0), "spmm_w")
            self.verify("spmm_csr_w", out=spmm(g, d.v0, d.Y, d.out0))
            # fused: the overwrite of Out belongs to the first window, the row epilogue to the last
            for flags, use_sv, epi in ((VOW | OOW | LEAKY, True, True), (0, False, False), (VOW, True, True)):
                self.reset()
                for q in range(nw):
                    last = q == nw - 1
                    ex = K.FusedExtras(ALPHA, X_SCALE if (epi and last) else 0.0, self.p("rowdot") if (epi and last) else None, None, None, 0)
                    f = flags if q == 0 else flags & ~OOW
                    c.check(lib.hnh_fused_sddmm_spmm_csr_w(c.h, g.rows, self.p("rowptr"), self.p("colidx"), self.p("values"), self.p("sv") if use_sv else None,
                                                           self.p("X"), self.p("Y"), self.p("out"), self.R, f, g.nnz, g.max_row, C.byref(ex),
                                                           C.byref(window(q)), 0), "fused_w")
                vals, out, dot = fused(g, d.v0, d.sv if use_sv else None, d.X, d.Y, d.out0, flags, ALPHA, X_SCALE if epi else 0.0, epi)
                outs = dict(values=vals, out=out)
                if epi:
                    outs["rowdot"] = dot
                self.verify("fused_csr_w flags=%d svalues=%s epilogue=%s" % (flags, use_sv, epi), **outs)
        finally:
            del self.a["split"]
            split.free()


def run(ctx, g, R, align, what):
    """one Block, one of its operation lists, freed whatever happens"""
    b = Block(ctx, g, data_for(g, R), align)
    try:
        what(b)
    finally:
        b.free()


# ------------------------------------------------------------------------------------------------ the expected-instance table
# Instances are named as the kernel templates are: (OP, LPR, VEC, W, EXACT, NARROW) with OP 0 = SDDMM, 1 = SpMM, 2 = fused.  Read off
# pick_shape / launch_shape / dispatch_row / fused_impl of csrc/hip/hnh_kernels.hip.
SDDMM, SPMM, FUSED = 0, 1, 2
SLAB_MIN_R = 320


def pick_shape(R, vec_ok):
    """-> (lpr, vec, w, exact)"""
    if R % 2 == 0 and vec_ok:
        ch = R // 2
        if ch <= 64 and ch & (ch - 1) == 0:
            return ch, 1, 2, True
        if ch % 64 == 0 and ch // 64 <= 4:
            return 64, ch // 64, 2, True
        if ch % 32 == 0 and ch // 32 in (3, 5, 7):
            return 32, ch // 32, 2, True
        return 64, 1, 2, False
    return 64, 1, 1, False


def _one_pass(op, R, shape, narrow):
    """launch_shape: the instance of one launch over whole dense rows, or None when R needs column tiles"""
    lpr, vec, w, exact = shape
    if exact:
        return (op, lpr, vec, 2, True, bool(narrow and lpr in (4, 8, 16) and vec == 1))
    for v in (1, 2, 4):
        if R <= 64 * w * v:
            return (op, 64, v, w, False, False)
    return None


def expected_instances(op, R, align="a16", narrow_rows=True, wide_slabs=True):
    """The row_kernel instances a whole-block public call of `op` launches at width R (long_row_kernel runs the same instance on the hub
    rows).  The fused pass at a width without a one-pass instance is composed of the tiled SDDMM and SpMM (fused_impl)."""
    shape = pick_shape(R, align != "dense8")
    lpr, vec, w, exact = shape
    narrow = narrow_rows and align != "csr1"
    if op == FUSED:
        if exact or R <= 256 * w:
            return {_one_pass(FUSED, R, shape, narrow)}
        return expected_instances(SDDMM, R, align, narrow_rows, wide_slabs) | expected_instances(SPMM, R, align, narrow_rows, wide_slabs)
    if wide_slabs and w == 2 and R >= SLAB_MIN_R and R % 64 == 0:  # 128-column slabs, a last one of 64
        return {(op, 64, 1, 2, True, False)} | ({(op, 32, 1, 2, True, False)} if R % 128 else set())
    one = _one_pass(op, R, shape, narrow)
    return {one} if one is not None else {(op, 64, 1, w, False, False)}


def expected_table():
    """every instance the GPU file is expected to launch -> the (width, alignment, switch) cases that reach it"""
    table = {}
    cases = [(R, a, True, True, "") for R, a in WIDTH_CASES]
    cases += [(R, "a16", False, True, "HNH_NARROW_ROWS=0") for R in W_SWITCHES] + [(R, "a16", True, False, "HNH_WIDE_SLABS=0") for R in W_SWITCHES + [320, 384, 512]]
    for R, a, narrow, slabs, tag in cases:
        for op in (SDDMM, SPMM, FUSED):
            for inst in expected_instances(op, R, a, narrow, slabs):
                table.setdefault(inst, []).append(("R%d %s %s" % (R, a, tag)).strip())
    return table


def instance_name(inst):
    """as a kernel trace prints the template arguments"""
    op, lpr, vec, w, exact, narrow = inst
    return "((anonymous namespace)::Op)%d, %d, %d, %d, %s, %s" % (op, lpr, vec, w, "true" if exact else "false", "true" if narrow else "false")
