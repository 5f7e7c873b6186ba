"""What the GAT's GPU test files share: the fixtures, the blocks and operands of the kernel tests, and the operator on loopback ranks
(setup / one_round / teardown, one reference, one assemble, one compare, one device sgd).  The numpy definitions are tests/gat_ref.py
(the model) and tests/gat_pass_ref.py (single passes).  Test modules import the fixtures by name (hip_backend is autouse in each)."""
import ctypes as C

import numpy as np
import pytest

import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from oracle import oracle as O

ALPHA = T.GAT_ALPHA
FTOL = 1e-12  # a forward kernel against the extended-precision reference
TOL = 1e-10   # backward kernels, the operator
NWIN = 6
GROUPINGS = {"whole": None, "one call per window": [(q, q + 1) for q in range(NWIN)], "uneven a": [(0, 1), (1, 4), (4, 6)],
             "uneven b": [(0, 3), (3, 4), (4, 5), (5, 6)]}
FWD, ROW, COL = 0, 1, 2
PASS_NAMES = {FWD: "fwd", ROW: "row", COL: "col"}


@pytest.fixture(autouse=True, scope="module")
def hip_backend():
    assert H.load_backend(None) == "hip-gfx950"  # fails loudly if the HIP library is missing
    yield


@pytest.fixture(scope="module")
def ctx():
    c = K.Ctx(0)
    assert K.load().hnh_backend_name() == b"hip-gfx950"
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ blocks
def graph(m, ncols, degrees, seed, repeat=True):
    """CSR (sorted columns, repeated pairs kept) with the given row lengths over ncols columns: (rowptr, colidx, the nonzeros' rows).
    repeat=True plants a repeated (i, j) pair for certain."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m), degrees)
    cols = rng.integers(0, ncols, len(rows))
    if repeat:
        first = int(np.nonzero(degrees >= 2)[0][0])
        beg = int(np.cumsum(degrees)[first] - degrees[first])
        cols[beg + 1] = cols[beg]
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int32)
    if repeat:
        pairs = rows.astype(np.int64) * ncols + cols
        assert len(np.unique(pairs)) < len(pairs)
    return rowptr, cols.astype(np.int32), rows


def square_graph(m, degrees, seed):
    """graph() over m columns without the planted pair: the blocks of the dot-product softmax tests"""
    return graph(m, m, degrees, seed, repeat=False)


def mixed_degrees(m, seed, empty=(3,)):
    """Rows of length 0 .. 40 (a fifth of them empty, and the rows of `empty`), a few of 200 .. 300 and hub rows past every long-row
    threshold (600, 1500)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 41, m)
    d[rng.random(m) < 0.2] = 0
    d[5::97] = rng.integers(200, 301, len(d[5::97]))
    d[7] = 600
    d[m // 2] = 1500
    d[list(empty)] = 0
    return d


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def errors(got, want):
    return {k: float(T.rel(np.asarray(got[k], dtype=np.longdouble), want[k])) for k in want}


# ------------------------------------------------------------------------------------------------ the dot-product softmax pass
def softmax_pass(ctx, rowptr, colidx, x, y, alpha, groups=None, nwin=6, off=2):
    """One softmax pass through hnh_attn_softmax_csr_p.  groups = None: one call over whole rows; else a list of (first, end) window
    ranges covering [0, nwin) of nwin column windows, one call each.  The head's block starts at column `off` of a relu_dst of pitch
    R + 4 (an odd off: 8-byte aligned only, the W = 1 instances).  Returns (relu output, lse, row_max, row_sum, values)."""
    lib = ctx.lib
    m, R_ = x.shape
    nnz = int(rowptr[-1])
    ld = R_ + 4
    drp, dci = ctx.upload(rowptr), ctx.upload(np.concatenate([colidx, [0]]).astype(np.int32))
    dx, dy = ctx.upload(x), ctx.upload(y)
    out = K.DevArray(ctx, m * R_, np.float64)
    vals = ctx.upload(np.full(max(nnz, 1), 3.0))
    rmax, rsum, lse = (ctx.upload(np.full(m, 5.0)) for _ in range(3))
    dst = ctx.upload(np.full((m, ld), 7.0))
    blk = K.CsrBlock(m, nnz, m, int(np.diff(rowptr).max()), 0, drp.ptr, dci.ptr, None)
    st = K.AttnState(rmax.ptr, rsum.ptr, lse.ptr, alpha, dst.ptr + off * 8, ld)
    base = K.FUSED_VALUES_OVERWRITE
    if groups is None:
        ctx.check(lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), vals.ptr, dx.ptr, dy.ptr, out.ptr, R_, base | K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH,
                                             C.byref(st), None, K.STREAM_COMPUTE), "softmax pass")
    else:
        bounds = (C.c_int32 * (nwin - 1))(*[int(m * (b + 1) / nwin) for b in range(nwin - 1)])
        split = K.DevArray(ctx, (nwin - 1) * m, np.int32)
        ctx.check(lib.hnh_csr_window_bounds(ctx.h, m, drp.ptr, dci.ptr, nwin - 1, bounds, split.ptr, K.STREAM_COMPUTE), "window bounds")
        for k, (a, b) in enumerate(groups):
            win = K.CsrWindow(None if a == 0 else split.ptr + (a - 1) * m * 4, None if b == nwin else split.ptr + (b - 1) * m * 4, int(b == nwin))
            flags = base | (K.FUSED_OUT_OVERWRITE if k == 0 else 0) | (K.ATTN_FINISH if b == nwin else 0)
            ctx.check(lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), vals.ptr, dx.ptr, dy.ptr, out.ptr, R_, flags, C.byref(st), C.byref(win),
                                                 K.STREAM_COMPUTE), "softmax window")
        split.free()
    ctx.sync()
    d = dst.get()
    assert np.all(d[:, :off] == 7.0) and np.all(d[:, off + R_:] == 7.0), "columns outside the head's block are not written"
    res = (d[:, off:off + R_], lse.get(), rmax.get(), rsum.get(), vals.get()[:nnz])
    for a in (drp, dci, dx, dy, out, vals, rmax, rsum, lse, dst):
        a.free()
    return res


def check_against_numpy(got, rows, colidx, m, x, y, sels=None):
    """The pass against the extended-precision reference (gat_pass_ref.attention_ld): output, lse, scores and the row state.  sels =
    boolean row masks: the output and lse bounds hold over each group of rows on its own (groups whose scales differ)."""
    o, lse, s = (np.float64(v) for v in P.attention_ld(rows, colidx.astype(np.int64), m, x, y, ALPHA))
    live = np.bincount(rows, minlength=m) > 0
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    for sel in (sels if sels is not None else [np.ones(m, dtype=bool)]):
        assert T.rel(got[0][sel], np.maximum(o[sel], 0.0)) <= 1e-12, T.rel(got[0][sel], np.maximum(o[sel], 0.0))
        assert np.max(np.abs(got[1][sel] - lse[sel])) <= 1e-12 * max(1.0, np.abs(lse[sel]).max()) and np.all(got[1][~live] == 0.0)
    assert T.rel(got[4], s) <= 1e-13
    assert np.all(got[2][~live] == -np.inf) and np.all(got[3][~live] == 0.0)
    mx = np.full(m, -np.inf)
    np.maximum.at(mx, rows, s)
    assert np.max(np.abs(got[2][live] - mx[live]), initial=0.0) <= 1e-13 * max(1.0, np.abs(s).max()) and np.all(got[3][live] >= 1.0)


# ------------------------------------------------------------------------------------------------ the additive passes
class Problem:
    """One additive pass's operands on the device, with pitches wider than the widths and guards round every output: run() launches the
    pass (whole block, or one call per window group) and returns its outputs.  odd=True puts the output block (the ReLU destination of
    the forward pass, dAgg of the column pass) at an odd column offset of an odd pitch and dZ at an odd pitch: the 8-byte instances.
    big > 0 scales a1, a2 so that |z| reaches about `big`."""
    ref_drop = None

    def __init__(self, ctx, pas, f, m=2048, ncols=1536, seed=0, odd=False, big=0.0, degrees=None):
        self.ctx, self.pas, self.f, self.m, self.ncols, self.odd = ctx, pas, f, m, ncols, odd
        fp = self.fp = f + (f & 1)
        rng = np.random.default_rng(1000 * f + seed + 17 * pas)
        deg = mixed_degrees(m, seed + f) if degrees is None else degrees
        self.rowptr, self.colidx, self.rows = graph(m, ncols, deg, seed + 1)
        rows, cols = self.rows, self.colidx.astype(np.int64)
        a1, a2 = rng.standard_normal(f) / np.sqrt(f), rng.standard_normal(f) / np.sqrt(f)
        a_rows, a_cols = rng.uniform(-1, 1, (m, f)), rng.uniform(-1, 1, (ncols, f))
        if big:
            z0 = ((a_cols @ a1)[cols] + (a_rows @ a2)[rows]) if pas == COL else ((a_rows @ a1)[rows] + (a_cols @ a2)[cols])
            scale = big / np.abs(z0).max()  # (z is linear in (a1, a2))
            a1, a2 = a1 * scale, a2 * scale
        self.a1, self.a2 = a1, a2
        self.ld_m, self.ld_y = fp + 4, (fp + 2 if pas != COL else fp + 4) + 4
        # S-row side and S-column side of the scores: for FWD / ROW the block's rows are S rows (s_i) and the gathered rows S columns
        # (t_j); for COL the block's rows are S columns (t_j) and the gathered rows S rows (s_i, lse_i, delta_i)
        self.m_rows = P.scored(a_rows, a1, a2, ld=self.ld_m)
        m_cols = P.scored(a_cols, a1, a2, ld=self.ld_y)
        s_nz = (m_cols[cols, fp] + self.m_rows[rows, fp + 1]) if pas == COL else (self.m_rows[rows, fp] + m_cols[cols, fp + 1])
        self.z = s_nz
        owner, n_own = (cols, ncols) if pas == COL else (rows, m)
        _, lse = R.row_softmax(owner, n_own, R.leaky(s_nz, ALPHA))
        self.lse_in = lse
        self.delta = rng.uniform(-1, 1, n_own)
        self.ld_dz = f + (3 if odd else 2 + (f & 1))
        self.dz = rng.uniform(-1, 1, (m, self.ld_dz))
        if pas == COL:
            self.dz_cols = rng.uniform(-1, 1, (ncols, f))
            self.y = P.pack(self.dz_cols, m_cols[:, fp], lse, self.delta, ld=self.ld_y)
        else:
            self.y = m_cols
        self.y = np.where(np.isnan(self.y), 1e300, self.y)       # beyond the gathered width: never read
        self.m_rows = np.where(np.isnan(self.m_rows), 1e300, self.m_rows)
        # outputs: a matrix of m + 1 rows whose block [col0, col0 + f) is the pass's, everything else a guard
        self.col0 = 3 if odd else 2
        self.ld_out = self.col0 + f + (4 if (self.col0 + f) % 2 == 0 else 3) + (1 if odd else 0)
        if not odd:
            assert self.ld_out % 2 == 0
        self.out0 = rng.uniform(-1, 1, (m + 1, self.ld_out))
        self.vec0 = rng.uniform(-1, 1, (m + 1, 2))
        self.state0 = rng.uniform(1, 2, (4, m + 1))  # row_max, row_sum, lse, (unused)
        self.acc0 = rng.uniform(-1, 1, (m + 1, fp + 2))  # the forward pass's running accumulator (scratch of the pass)
        host = dict(rowptr=self.rowptr, colidx=np.concatenate([self.colidx, [0]]).astype(np.int32), m_rows=self.m_rows, dz=self.dz, y=self.y,
                    out=self.out0, vec=self.vec0, state=self.state0, acc=self.acc0, lse_in=self.lse_in if pas == ROW else np.zeros(1),
                    delta=self.delta if pas == ROW else np.zeros(1))
        self.d = {k: ctx.upload(v) for k, v in host.items()}
        self.split = None

    def args(self):
        d, m, f = self.d, self.m, self.f
        a = K.AttnAdd()
        a.M, a.ld_m, a.Y, a.ld_y, a.f, a.leaky_alpha = d["m_rows"].ptr, self.ld_m, d["y"].ptr, self.ld_y, f, ALPHA
        if self.pas == FWD:
            a.Out, a.ld_out = d["acc"].ptr, self.fp + 2
            a.row_max, a.row_sum, a.lse = d["state"].ptr, d["state"].ptr + 8 * (m + 1), d["state"].ptr + 16 * (m + 1)
            a.relu_dst, a.relu_ld = d["out"].ptr + 8 * self.col0, self.ld_out
        elif self.pas == ROW:
            a.dZ, a.ld_dz, a.lse, a.delta = d["dz"].ptr, self.ld_dz, d["lse_in"].ptr, d["delta"].ptr
            a.vec, a.ld_vec = d["vec"].ptr, 2
        else:
            a.Out, a.ld_out = d["out"].ptr + 8 * self.col0, self.ld_out
            a.vec, a.ld_vec = d["vec"].ptr + 8, 2
        return a

    def block(self):
        return K.CsrBlock(self.m, int(self.rowptr[-1]), self.ncols, int(np.diff(self.rowptr).max()), 0, self.d["rowptr"].ptr, self.d["colidx"].ptr, None)

    def fn(self):
        lib = self.ctx.lib
        return (lib.hnh_attn_add_fwd_csr_p, lib.hnh_attn_add_row_csr_p, lib.hnh_attn_add_col_csr_p)[self.pas]

    def run(self, overwrite=True, groups=None):
        """Returns dict(out=block rows x f, vec=rows, lse=rows, state=(max, sum)) as far as the pass writes them; checks the guards."""
        ctx, lib, m, f = self.ctx, self.ctx.lib, self.m, self.f
        for k, v in (("out", self.out0), ("vec", self.vec0), ("state", self.state0), ("acc", self.acc0)):
            self.d[k].set(v)
        a, blk = self.args(), self.block()
        first = K.FUSED_OUT_OVERWRITE if (overwrite or self.pas == FWD) else 0
        finish = K.ATTN_FINISH if self.pas == FWD else 0
        if groups is None:
            ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), first | finish, None, K.STREAM_COMPUTE), "additive pass")
        else:
            if self.split is None:
                bounds = (C.c_int32 * (NWIN - 1))(*[int(self.ncols * (b + 1) / NWIN) for b in range(NWIN - 1)])
                self.split = K.DevArray(ctx, (NWIN - 1) * m, np.int32)
                ctx.check(lib.hnh_csr_window_bounds(ctx.h, m, self.d["rowptr"].ptr, self.d["colidx"].ptr, NWIN - 1, bounds, self.split.ptr,
                                                    K.STREAM_COMPUTE), "window bounds")
            sp = self.split.ptr
            for k, (w0, w1) in enumerate(groups):
                win = K.CsrWindow(None if w0 == 0 else sp + (w0 - 1) * m * 4, None if w1 == NWIN else sp + (w1 - 1) * m * 4, int(w1 == NWIN))
                fl = (first if k == 0 else 0) | (finish if w1 == NWIN else 0)
                ctx.check(self.fn()(ctx.h, C.byref(blk), C.byref(a), fl, C.byref(win), K.STREAM_COMPUTE), "additive window")
        ctx.sync()
        out, vec, state = self.d["out"].get(), self.d["vec"].get(), self.d["state"].get()
        c0 = self.col0
        res = {}
        if self.pas != ROW:
            assert np.array_equal(out[:, :c0], self.out0[:, :c0]) and np.array_equal(out[:, c0 + f:], self.out0[:, c0 + f:]), "guard columns are not written"
            assert np.array_equal(out[m], self.out0[m]), "the row past the last one is not written"
            res["out"] = out[:m, c0:c0 + f]
        else:
            assert np.array_equal(out, self.out0)
        if self.pas == FWD:
            assert np.array_equal(vec, self.vec0) and np.array_equal(state[:, m], self.state0[:, m]) and np.array_equal(state[3], self.state0[3])
            res["lse"], res["state"] = state[2, :m], state[:2, :m]
        else:
            col = 0 if self.pas == ROW else 1
            assert np.array_equal(vec[:, 1 - col], self.vec0[:, 1 - col]) and np.array_equal(vec[m], self.vec0[m]), "the other scalar column is not written"
            assert np.array_equal(state, self.state0)
            res["vec"] = vec[:m, col]
        return res

    def raw(self):
        """(o, lse) of the forward pass in np.longdouble, before the activation"""
        return P.fwd_pass_ld(self.rows, self.colidx.astype(np.int64), self.m, self.m_rows, self.y, self.f, ALPHA, self.ref_drop)

    def want(self, overwrite=True):
        f, m, cols = self.f, self.m, self.colidx.astype(np.int64)
        if self.pas == FWD:
            o, lse = self.raw()
            return dict(out=np.maximum(o, 0), lse=lse)
        if self.pas == ROW:
            ds = P.row_pass(self.rows, cols, m, self.dz[:, :f], self.m_rows, self.lse_in, self.delta, self.y, f, ALPHA, self.ref_drop)
            return dict(vec=ds + (0 if overwrite else self.vec0[:m, 0]))
        dagg, dt = P.col_pass(self.rows, cols, m, self.m_rows, self.y, f, ALPHA, self.ref_drop)
        if not overwrite:
            dagg, dt = dagg + self.out0[:m, self.col0:self.col0 + f], dt + self.vec0[:m, 1]
        return dict(out=dagg, vec=dt)

    def free(self):
        for v in self.d.values():
            v.free()
        if self.split is not None:
            self.split.free()


class DropProblem(Problem):
    """Problem with the ids in the gathered operand (M' for the forward and the row pass, Q' for the column pass) and the DROP entry
    points.  Own rows are row_id0 + r with row_id0 just below 2^31, so they cross it; gathered rows carry a scattered relabelling that
    reaches beyond 2^31 as well."""

    def __init__(self, ctx, pas, f, seed=0, drop_seed=0xC0FFEE1234567890, p=0.6, **kw):
        super().__init__(ctx, pas, f, seed=seed, **kw)
        fp = self.fp
        self.row_id0 = (1 << 31) - self.m // 2
        rng = np.random.default_rng(99 + f + seed)
        self.ids = rng.permutation(np.arange(self.ncols, dtype=np.int64) * 2700001 + 17)  # distinct, scattered over [17, 4.2e9)
        assert self.ids.max() < 1 << 32 and self.ids.max() >= 1 << 31
        if pas == COL:
            self.y[:, fp + 3] = self.ids
        else:
            assert self.ld_y >= fp + 4
            self.y[:, fp + 2], self.y[:, fp + 3] = self.ids, 0.0
        self.d["y"].set(self.y)
        self.drop = K.AttnDrop(drop_seed, 2 * 65536 + 5, K.dropout_threshold(p), 1.0 / (1.0 - p), self.row_id0)
        self.ref_drop = (drop_seed, 2 * 65536 + 5, p, self.row_id0)

    def fn(self):
        lib = self.ctx.lib
        f = (lib.hnh_attn_drop_fwd_csr_p, lib.hnh_attn_drop_row_csr_p, lib.hnh_attn_drop_col_csr_p)[self.pas]
        return lambda h, blk, a, flags, win, stream: f(h, blk, a, C.byref(self.drop), flags, win, stream)

    def factor(self):
        """c m per nonzero"""
        cols = self.colidx.astype(np.int64)
        own = self.rows.astype(np.uint64) + np.uint64(self.row_id0)
        got = self.ids[cols].astype(np.uint64)
        seed, w2, p, _ = self.ref_drop
        gi, gj = (got, own) if self.pas == COL else (own, got)
        return P.keep(seed, 0, w2, gi, gj, p) / (1.0 - p)


# ------------------------------------------------------------------------------------------------ the operator on loopback ranks
def er8():
    case = T.case_inputs("er8_r16")
    return case["rows"], case["cols"], case["M"], case["A"] * T.GAT_INPUT_SCALE


def hashed_weights(layers, scale_later=1.0):
    """The hashed weights of oracle.gat_weight; scale_later lifts the layers after the first (without a softmax their inputs
    are small)."""
    return {(li, h): O.gat_weight(li, h, fin, fph) * (1.0 if li == 0 else scale_later) for li, (fin, fph, heads) in enumerate(layers) for h in range(heads)}


def setup(world, rows, cols, m, x, layers, weights, vectors, g_glob=None, alg="15d_fusion2", c=1, **kw):
    """One rank's operator with its parameters, input, dL/d(output) and result buffers; **kw goes to H.GAT."""
    sp = H.SpmatLocal.from_global(world, m, m, rows, cols, np.ones(len(rows)))
    d = H.DistributedSparse(world, alg, sp, layers[0][0], c)
    gnn = H.GAT(d, layers, ALPHA, **kw)
    for k, w in weights.items():
        gnn.set_weight(*k, w)
    if vectors is not None:
        for k, (a1, a2) in vectors.items():
            gnn.set_attention_vectors(*k, a1, a2)
    d.setRValue(layers[0][0])
    subB = d.submatrices(H.BMAT)
    d.setRValue(layers[-1][1] * layers[-1][2])
    subA = d.submatrices(H.AMAT)
    x_d = H.Dense.create(world, *gnn.buffer_shape(0))
    x_d.upload(T.fill_local(subB, x_d.shape, x))
    g = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
    if g_glob is not None:
        g.upload(T.fill_local(subA, g.shape, g_glob))
    out = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
    dx = H.Dense.create(world, *gnn.buffer_shape(0))
    gnn.set_input(x_d)
    return dict(sp=sp, d=d, gnn=gnn, x=x_d, g=g, out=out, dx=dx, subA=subA, subB=subB)


def one_round(s, weights, additive, forward=True, out_after=False):
    """forwardPass (unless forward=False: the stored one), the output, backwardPass, every gradient; out_after=True reads the output
    again after the backward pass."""
    gnn = s["gnn"]
    if forward:
        gnn.forwardPass()
    gnn.get_output(s["out"])
    r = dict(out=s["out"].download())
    gnn.backwardPass(s["g"])
    if out_after:
        gnn.get_output(s["out"])
        r["out_after"] = s["out"].download()
    gnn.get_input_grad(s["dx"])
    r.update(dx=s["dx"].download(), dw={k: gnn.weight_grad(*k) for k in weights})
    if additive:
        r["da"] = {k: gnn.attention_grad(*k) for k in weights}
    return r


def teardown(s):
    for k in ("x", "g", "out", "dx", "gnn", "d", "sp"):
        s[k].free()


def run_rounds(world, rows, cols, m, x, layers, weights, vectors, g_glob, rounds=1, out_after=False, **kw):
    """`rounds` forward + backward rounds of one object: this rank's blocks and every round's results."""
    s = setup(world, rows, cols, m, x, layers, weights, vectors, g_glob, **kw)
    res = dict(subA=s["subA"], subB=s["subB"], rounds=[one_round(s, weights, vectors is not None, out_after=out_after) for _ in range(rounds)])
    teardown(s)
    return res


def reference(rows, cols, m, x, layers, w, av, g, **mode):
    """dict(out, dw, da, dx) of the numpy definition"""
    dw, da, dx = R.backward(rows, cols, m, x, layers, ALPHA, g, w, av, **mode)
    return dict(out=R.forward(rows, cols, m, x, layers, ALPHA, w, av, **mode), dw=dw, da=da, dx=dx)


def assembled(per_rank, k, m, layers):
    """The global output and dX of round k, and rank 0's replicated gradients (asserted equal on every rank)."""
    r0 = per_rank[0]["rounds"][k]
    for pr in per_rank:
        for key in r0["dw"]:
            assert np.array_equal(pr["rounds"][k]["dw"][key], r0["dw"][key]), "dW must be equal on every rank"
            assert all(np.array_equal(pr["rounds"][k]["da"][key][i], r0["da"][key][i]) for i in (0, 1) if "da" in r0), "da1, da2 must be equal on every rank"
    hf = layers[-1][1] * layers[-1][2]
    out = T.assemble_dense([dict(o=pr["rounds"][k]["out"], subA=pr["subA"]) for pr in per_rank], "o", "subA", m, hf)
    dx = T.assemble_dense([dict(dx=pr["rounds"][k]["dx"], subB=pr["subB"]) for pr in per_rank], "dx", "subB", m, layers[0][0])
    return dict(out=out, dx=dx, dw=r0["dw"], da=r0.get("da", {}))


def compare(got, want, kind, label, ranks, check=("out", "dw", "da", "dx"), tol=TOL):
    """The matrices of `check` (dw, da: of every (layer, head)) against the reference, max |x - ref| / max |ref| each; every gradient
    compared must not be vacuous; the worst is recorded under `kind` and asserted <= tol."""
    errs = {name: T.rel(got[name], want[name]) for name in ("out", "dx") if name in check}
    for key in (want["dw"] if "dw" in check else ()):
        assert np.abs(want["dw"][key]).max() > 0
        errs[("dw",) + key] = T.rel(got["dw"][key], want["dw"][key])
    for key in (want["da"] if "da" in check else ()):
        for i in (0, 1):
            assert np.abs(want["da"][key][i]).max() > 0
            errs[("da%d" % (i + 1),) + key] = T.rel(got["da"][key][i], want["da"][key][i])
    worst = max(errs.values())
    T.record_observed(kind, case=label, ranks=ranks, worst=worst)
    print("observed", kind, label, ranks, "worst %.2e" % worst)
    assert worst <= tol, errs


def sgd(world, rows, cols, m, x, layers, target, steps, lr_scale, w, av=None, **kw):
    """steps of plain gradient descent on L = 1/2 |out - target|^2 over W (and a1, a2 when given), as gat_ref.descend does them: returns
    (this rank's share of L before every step and after the last, the final vectors).  **kw goes to setup."""
    w, av = dict(w), dict(av or {})
    s = setup(world, rows, cols, m, x, layers, w, av, None, **kw)
    gnn = s["gnn"]
    tgt = T.fill_local(s["subA"], gnn.buffer_shape(len(layers)), target)
    losses, lr = [], None
    for step in range(steps + 1):
        gnn.forwardPass()
        gnn.get_output(s["out"])
        diff = s["out"].download() - tgt
        losses.append(0.5 * float(np.sum(diff * diff)))
        if step == steps:
            break
        s["g"].upload(diff)
        gnn.backwardPass(s["g"])
        dw = {k: gnn.weight_grad(*k) for k in w}
        da = {k: gnn.attention_grad(*k) for k in av}
        if lr is None:  # the same on every rank: the gradients are replicated
            lr = R.sgd_step_size(lr_scale, w, av, dw, da)
        for k in w:
            w[k] = w[k] - lr * dw[k]
            gnn.set_weight(*k, w[k])
        for k in av:
            av[k] = (av[k][0] - lr * da[k][0], av[k][1] - lr * da[k][1])
            gnn.set_attention_vectors(*k, *av[k])
    teardown(s)
    return losses, av
