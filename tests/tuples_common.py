"""Shared body of the setup-primitive tests (hnh_tuples_* of include/hnh_kernels.h): the same checks run against the
oracle's C test double on the CPU and against the HIP library on the GPU; expectations are plain numpy."""
import ctypes as C

import numpy as np

from distributed_sddmm_amd import _kernels as K


def make_tuples(n, rows, cols, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=K.TUPLE_DTYPE)
    t["r"], t["c"] = rng.integers(0, rows, n), rng.integers(0, cols, n)
    t["value"] = rng.uniform(-1, 1, n)
    return t


def key_of(t, kind, **kw):
    r, c = t["r"].astype(np.uint64), t["c"].astype(np.uint64)
    if kind == K.KEY_ROW_COL:
        return (r << np.uint64(32)) | c
    if kind == K.KEY_COL_ROW:
        return (c << np.uint64(32)) | r
    if kind == K.KEY_OWNER:
        rr, cc = (c, r) if kw["transpose"] else (r, c)
        return kw["table"][(rr // np.uint64(kw["rib"])) * np.uint64(kw["ncb"]) + cc // np.uint64(kw["cib"])].astype(np.uint64)
    return c // np.uint64(kw["div"])


def run(api):
    """api: object with upload(np)->handle(.ptr,.get(),.free()), lib, ctx handle `h`, check(rc, what)."""
    lib, h = api.lib, api.h
    rows, cols, n = 1000, 777, 50000
    t0 = make_tuples(n, rows, cols, 3)
    table = np.random.default_rng(4).integers(0, 8, 10 * 7).astype(np.int32)  # 10 x 7 blocks of 100 x 111, 8 owners
    dtab = api.upload(table)
    cases = [(K.KEY_ROW_COL, {}, 64), (K.KEY_COL_ROW, {}, 32 + 10), (K.KEY_COL_DIV, dict(div=100), 4),
             (K.KEY_OWNER, dict(transpose=0, rib=100, cib=111, ncb=7, table=table), 3),
             (K.KEY_OWNER, dict(transpose=1, rib=111, cib=100, ncb=10, table=table), 3)]
    for kind, kw, bits in cases:
        if kind == K.KEY_OWNER and kw["transpose"]:  # 7 x 10 blocks over the transposed matrix
            kw["table"] = table[:70]
        key = K.TupleKey(kind, kw.get("transpose", 0), kw.get("rib", 0), kw.get("cib", 0), kw.get("ncb", 0), dtab.ptr, kw.get("div", 0))
        d = api.upload(t0)
        api.check(lib.hnh_tuples_sort(h, d.ptr, n, C.byref(key), bits, 0), "tuples_sort")
        got = d.get().view(K.TUPLE_DTYPE).reshape(-1)
        order = np.argsort(key_of(t0, kind, **kw), kind="stable")   # the sort is stable
        assert np.array_equal(got, t0[order]), "kind %d" % kind
        # boundaries
        nb = int(key_of(t0, kind, **kw).max()) + 1 if kind in (K.KEY_OWNER, K.KEY_COL_DIV) else 5
        starts = np.zeros(nb + 1, dtype=np.int64)
        api.check(lib.hnh_tuples_bucket_starts(h, d.ptr, n, C.byref(key), nb, starts.ctypes.data_as(C.c_void_p), 0), "bucket_starts")
        want = np.searchsorted(key_of(got, kind, **kw), np.arange(nb + 1, dtype=np.uint64), side="left")
        assert np.array_equal(starts, want)
        d.free()
    # transform: swap, then mod
    d = api.upload(t0)
    api.check(lib.hnh_tuples_transform(h, d.ptr, n, 1, 13, 0, 0), "transform")
    got = d.get().view(K.TUPLE_DTYPE).reshape(-1)
    assert np.array_equal(got["r"], t0["c"] % 13) and np.array_equal(got["c"], t0["r"]) and np.array_equal(got["value"], t0["value"])
    d.free()
    # remap_cols: segment (c / div) * n_sub + (c % div) / sub_div moves to dest[segment], offsets inside a segment stay
    div, sub, nsub = 100, 34, 3
    dest = np.random.default_rng(5).permutation(8 * nsub).astype(np.int64) * 1000   # 777 columns -> 8 blocks x 3 chunks
    d = api.upload(t0)
    api.check(lib.hnh_tuples_remap_cols(h, d.ptr, n, div, sub, nsub, dest.ctypes.data_as(C.c_void_p), len(dest), 0), "remap_cols")
    got = d.get().view(K.TUPLE_DTYPE).reshape(-1)
    c0 = t0["c"].astype(np.int64)
    seg = (c0 // div) * nsub + (c0 % div) // sub
    assert np.array_equal(got["c"].astype(np.int64), dest[seg] + (c0 % div) % sub) and np.array_equal(got["r"], t0["r"])
    # a tuple in a segment without destination (negative entry, or beyond the table) is an error
    bad = dest.copy(); bad[int(seg[0])] = -1
    d2 = api.upload(t0)
    assert lib.hnh_tuples_remap_cols(h, d2.ptr, n, div, sub, nsub, bad.ctypes.data_as(C.c_void_p), len(bad), 0) != 0
    assert lib.hnh_tuples_remap_cols(h, d2.ptr, n, div, sub, nsub, dest.ctypes.data_as(C.c_void_p), 3, 0) != 0
    d.free(); d2.free()
    # to_csr on de-duplicated (row, col)-ordered tuples, with empty rows and one hub row
    keys = np.unique(np.concatenate([key_of(t0, K.KEY_ROW_COL)[t0["r"] % 7 != 3], (np.uint64(5) << np.uint64(32)) | np.arange(cols, dtype=np.uint64)]))
    ts = np.zeros(len(keys), dtype=K.TUPLE_DTYPE)
    ts["r"], ts["c"], ts["value"] = keys >> np.uint64(32), keys & np.uint64(0xffffffff), np.arange(len(keys)) * 0.5
    d = api.upload(ts)
    drp, dci, dv = api.upload(np.zeros(rows + 1, np.int32)), api.upload(np.zeros(len(ts), np.int32)), api.upload(np.zeros(len(ts)))
    mx = C.c_int(-1)
    api.check(lib.hnh_tuples_to_csr(h, d.ptr, len(ts), rows, cols, drp.ptr, dci.ptr, dv.ptr, C.byref(mx), 0), "to_csr")
    want_rp = np.searchsorted(ts["r"], np.arange(rows + 1), side="left").astype(np.int32)
    assert np.array_equal(drp.get().reshape(-1), want_rp) and np.array_equal(dci.get().reshape(-1), ts["c"].astype(np.int32))
    assert np.array_equal(dv.get().reshape(-1), ts["value"]) and mx.value == int(np.diff(want_rp).max()) == cols
    # window bounds on that CSR block: first nonzero of every row with column >= bound
    bounds = np.array([0, 100, 100, 500, 776, 5000], dtype=np.int32)
    dsp = api.upload(np.zeros((len(bounds), rows), np.int32))
    api.check(lib.hnh_csr_window_bounds(h, rows, drp.ptr, dci.ptr, len(bounds), bounds.ctypes.data_as(C.c_void_p), dsp.ptr, 0), "window_bounds")
    ci = ts["c"].astype(np.int64)
    for b, bound in enumerate(bounds):
        want_split = np.array([want_rp[r] + np.searchsorted(ci[want_rp[r]:want_rp[r + 1]], bound, side="left") for r in range(rows)])
        assert np.array_equal(dsp.get().reshape(len(bounds), rows)[b], want_split.astype(np.int32))
    assert lib.hnh_csr_window_bounds(h, rows, drp.ptr, dci.ptr, 2, np.array([5, 3], np.int32).ctypes.data_as(C.c_void_p), dsp.ptr, 0) != 0
    dsp.free()
    # a tuple outside the block is an error, like the reference's MKL call would be
    assert lib.hnh_tuples_to_csr(h, d.ptr, len(ts), rows, cols - 1, drp.ptr, dci.ptr, dv.ptr, C.byref(mx), 0) != 0
    # empty input
    api.check(lib.hnh_tuples_to_csr(h, None, 0, 4, 4, drp.ptr, None, None, C.byref(mx), 0), "to_csr empty")
    assert np.array_equal(drp.get().reshape(-1)[:5], np.zeros(5, np.int32)) and mx.value == 0
    api.check(lib.hnh_tuples_sort(h, None, 0, C.byref(K.TupleKey(K.KEY_ROW_COL, 0, 0, 0, 0, None, 0)), 64, 0), "sort empty")
    # indices beyond 32 bits cannot be keyed
    big = t0[:10].copy(); big["r"][3] = 1 << 33
    db = api.upload(big)
    assert lib.hnh_tuples_sort(h, db.ptr, 10, C.byref(K.TupleKey(K.KEY_ROW_COL, 0, 0, 0, 0, None, 0)), 64, 0) != 0
    for x in (d, drp, dci, dv, dtab, db):
        x.free()
    run_generator(api)


def run_generator(api):
    """hnh_generate_er_keys / hnh_tuples_from_keys / hnh_tuples_relabel against oracle.py (the generator's numpy twin)."""
    from oracle import oracle as O
    lib, h = api.lib, api.h
    m, n, draws, seed = 300, 170, 4000, 99
    rows, cols = O.erdos_renyi_mn(m, n, draws, seed)
    dk = api.upload(np.zeros(draws, dtype=np.uint64))
    cnt = C.c_int64(-1)
    api.check(lib.hnh_generate_er_keys(h, m, n, draws, seed, dk.ptr, C.byref(cnt), 0), "generate_er_keys")
    assert cnt.value == len(rows) < draws  # duplicates were dropped
    keys = dk.get().reshape(-1)[:cnt.value]
    assert np.array_equal(keys, rows.astype(np.uint64) * np.uint64(n) + cols.astype(np.uint64))
    for rank, p in ((0, 1), (1, 3), (2, 3)):
        cnt_local = (cnt.value - rank + p - 1) // p
        dt = api.upload(np.zeros(cnt_local, dtype=K.TUPLE_DTYPE))
        api.check(lib.hnh_tuples_from_keys(h, dk.ptr, n, rank, p, 1.0, dt.ptr, cnt_local, 0), "tuples_from_keys")
        t = dt.get().view(K.TUPLE_DTYPE).reshape(-1)
        assert np.array_equal(t["r"], rows[rank::p].astype(np.uint64)) and np.array_equal(t["c"], cols[rank::p].astype(np.uint64))
        assert np.all(t["value"] == 1.0)
        rl, cl = O.vertex_permutation(m, 7).astype(np.uint64), O.vertex_permutation(n, 8).astype(np.uint64)
        drl, dcl = api.upload(rl), api.upload(cl)
        api.check(lib.hnh_tuples_relabel(h, dt.ptr, cnt_local, drl.ptr, dcl.ptr, 0), "tuples_relabel")
        t2 = dt.get().view(K.TUPLE_DTYPE).reshape(-1)
        assert np.array_equal(t2["r"], rl[rows[rank::p]]) and np.array_equal(t2["c"], cl[cols[rank::p]])
        for x in (dt, drl, dcl):
            x.free()
    dk.free()
    # the skewed initiator (hnh_generate_rmat_keys) against oracle.rmat, scrambled and not
    for logm, edges, abc, scramble in ((9, 6000, (0.57, 0.19, 0.19), 1), (7, 900, (0.45, 0.15, 0.15), 0), (10, 5000, (0.25, 0.25, 0.25), 1)):
        rows, cols = O.rmat(logm, edges, *abc, seed=77, scramble=bool(scramble))
        dk = api.upload(np.zeros(edges, dtype=np.uint64))
        cnt = C.c_int64(-1)
        api.check(lib.hnh_generate_rmat_keys(h, logm, edges, abc[0], abc[1], abc[2], 77, scramble, dk.ptr, C.byref(cnt), 0), "generate_rmat_keys")
        assert cnt.value == len(rows)
        assert np.array_equal(dk.get().reshape(-1)[:cnt.value], rows.astype(np.uint64) * np.uint64(1 << logm) + cols.astype(np.uint64))
        dk.free()
    cnt = C.c_int64(-1)
    assert lib.hnh_generate_rmat_keys(h, 9, 10, 0.6, 0.3, 0.3, 1, 1, None, C.byref(cnt), 0) != 0  # probabilities above one


def run_round6_primitives(api):
    """hnh_spmm_csr_pf (SpMM that STORES fresh output rows), hnh_sum_chunked_blocks_f64 (the closing step of the mesh reduce-scatter) and
    hnh_ctx_device_identity against numpy — the body the CPU test runs on the test double and the GPU test on the HIP library."""
    from oracle import oracle as O
    lib, h = api.lib, api.h
    rng = np.random.default_rng(5)
    # ---- SpMM with the store flag: rows without nonzeros end as zeros, garbage in Out is never read
    rows, cols, R = 90, 400, 48
    lens = rng.integers(0, 30, rows)
    lens[7] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cidx = np.concatenate([np.sort(rng.choice(cols, int(n), replace=False)) for n in lens]).astype(np.int32)
    vals, Y = rng.uniform(-1, 1, len(cidx)), rng.uniform(-1, 1, (cols, R))
    d_rp, d_c, d_v, dY = api.upload(rowptr), api.upload(cidx), api.upload(vals), api.upload(Y)
    blk = K.CsrBlock(rows, len(cidx), cols, int(lens.max()), 0, d_rp.ptr, d_c.ptr, None)
    want = O.spmm_local(rowptr, cidx, vals, Y, np.zeros((rows, R)))
    dOut = api.upload(np.full((rows, R), 1e300))
    api.check(lib.hnh_spmm_csr_pf(h, C.byref(blk), d_v.ptr, dY.ptr, dOut.ptr, R, K.FUSED_OUT_OVERWRITE, None, 0), "spmm_pf store")
    got = dOut.get().reshape(rows, R)
    assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want)) and np.all(got[7] == 0.0)
    out0 = rng.uniform(-1, 1, (rows, R))
    dOut2 = api.upload(out0)
    api.check(lib.hnh_spmm_csr_pf(h, C.byref(blk), d_v.ptr, dY.ptr, dOut2.ptr, R, 0, None, 0), "spmm_pf add")
    assert np.max(np.abs(dOut2.get().reshape(rows, R) - (out0 + want))) <= 1e-11 * np.max(np.abs(want))
    assert lib.hnh_spmm_csr_pf(h, C.byref(blk), d_v.ptr, dY.ptr, dOut2.ptr, R, 64, None, 0) != 0  # unknown flag
    # ---- the chunk-major sum, in block order (bit for bit)
    for R2, cuts in ((128, [0, 5, 5, 40, 77]), (7, [0, 3, 30]), (16, [0, 64])):
        nb, nrows = 5, cuts[-1]
        dst0, src = rng.uniform(-1, 1, (nrows, R2)), rng.uniform(-1, 1, (nb * nrows, R2))
        ch = np.array(cuts, dtype=np.int64)
        nch = len(cuts) - 1
        d_src = api.upload(src)
        for q0, q1 in ((0, nch), (1, nch), (0, 1)):
            d_dst = api.upload(dst0)
            api.check(lib.hnh_sum_chunked_blocks_f64(h, d_dst.ptr, d_src.ptr, nb, nch, ch.ctypes.data_as(C.c_void_p), q0, q1, R2, 0), "sum_chunked")
            want2 = dst0.copy()
            for q in range(q0, q1):
                w = cuts[q + 1] - cuts[q]
                for k in range(nb):
                    want2[cuts[q]:cuts[q + 1]] += src[nb * cuts[q] + k * w: nb * cuts[q] + (k + 1) * w]
            assert np.array_equal(d_dst.get().reshape(nrows, R2), want2)
            d_dst.free()
        d_src.free()
    bad = np.array([0, 5, 3], dtype=np.int64)
    assert lib.hnh_sum_chunked_blocks_f64(h, None, None, 2, 2, bad.ctypes.data_as(C.c_void_p), 0, 2, 8, 0) != 0  # cuts that decrease
    # ---- where the context runs
    ordinal, bus = C.c_int(-1), C.create_string_buffer(40)
    api.check(lib.hnh_ctx_device_identity(h, C.byref(ordinal), bus, 40), "device_identity")
    assert ordinal.value == 0 and len(bus.value) >= 7 and b":" in bus.value
    assert lib.hnh_ctx_device_identity(h, C.byref(ordinal), bus, 4) != 0  # a buffer too short for a bus id
    for x in (d_rp, d_c, d_v, dY, dOut, dOut2):
        x.free()


# ------------------------------------------------------------------------------------------------ the set-up primitives at their edges
# One body per primitive; every expectation is plain numpy and exact (tuples: on the raw bytes).  Each body takes the same `api` as run().
CAP = 8192 * 256   # grid_for of hnh_tuples.hip: at most 8192 workgroups of 256 threads, beyond that the grid-stride loops take a second trip
BIG = CAP + 257    # "beyond the cap": a second trip for 257 elements, i.e. one full workgroup and one thread of the next


def tuples_of(r, c, value):
    t = np.zeros(len(r), dtype=K.TUPLE_DTYPE)
    t["r"], t["c"], t["value"] = r, c, value
    return t


def fetch(d, n=None):
    return d.get().view(K.TUPLE_DTYPE).reshape(-1)[:n]


def same_bytes(got, want):
    """Bit for bit (the sign of a zero and the payload of an infinity included): the structured arrays compared as bytes."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def host_key_bits(dim):
    """The loop of the host callers (row_bits / col_bits in spmat_local.hpp, er_generator.cpp): the fewest bits that hold dim - 1."""
    bits = 1
    while bits < 32 and (1 << bits) < dim:
        bits += 1
    return bits


def host_owner_bits(p):
    """owner_bits of SpmatLocal::redistribute"""
    bits = 1
    while (1 << bits) < p:
        bits += 1
    return bits


def tuple_key(kind, transpose=0, rib=0, cib=0, ncb=0, table_ptr=None, div=0):
    return K.TupleKey(kind, transpose, rib, cib, ncb, table_ptr, div)


# ---- 1. dedup_max
def dedup_reference(t):
    if len(t) == 0:
        return t.copy()
    heads = np.flatnonzero(np.concatenate([[True], (t["r"][1:] != t["r"][:-1]) | (t["c"][1:] != t["c"][:-1])]))
    out = t[heads].copy()
    out["value"] = np.maximum.reduceat(t["value"], heads)
    return out


def check_dedup(api, t, what):
    want = dedup_reference(t)
    d = api.upload(t) if len(t) else None
    cnt = C.c_int64(-1)
    api.check(api.lib.hnh_tuples_dedup_max(api.h, d.ptr if d else None, len(t), C.byref(cnt), 0), "dedup_max " + what)
    assert cnt.value == len(want), (what, cnt.value, len(want))
    if d:
        assert same_bytes(fetch(d, cnt.value), want), what
        d.free()
    return want


def runs_to_tuples(heads, value):
    """Tuples in (r, c) order whose runs of equal coordinates begin where `heads` is set"""
    rid = np.cumsum(heads) - 1
    return tuples_of(rid // 1000, rid % 1000, value)


def dedup_max_beyond_cap(api):
    """hnh_tuples_dedup_max on CAP + 257 tuples: run lengths from {1, 1, 1, 2, 3, 7}, one run of 5000 from index 250 (many workgroups,
    one thread's walk), one run over CAP - 3 .. CAP + 3 (both trips of the grid-stride loop), +-inf among the values.  No NaN, and
    no run in which -0.0 and +0.0 tie for the maximum: there the double (`>`) and fmax may differ in the sign bit, which the contract
    ("the run's maximum value") leaves open."""
    rng = np.random.default_rng(21)
    n = BIG
    starts = np.concatenate([[0], np.cumsum(rng.choice([1, 1, 1, 2, 3, 7], n))])
    heads = np.zeros(n, dtype=bool)
    heads[starts[starts < n]] = True
    for a, b in ((250, 5250), (CAP - 3, CAP + 4)):
        heads[a], heads[a + 1:b], heads[b] = True, False, True
    value = rng.uniform(-1, 1, n)
    special = rng.choice(n, 100, replace=False)
    value[special[:50]], value[special[50:]] = np.inf, -np.inf
    assert not np.any(value == 0.0)
    t = runs_to_tuples(heads, value)
    want = check_dedup(api, t, "beyond the cap")
    lens = np.diff(np.flatnonzero(np.concatenate([heads, [True]])))
    assert lens.max() == 5000 and 7 in lens and len(want) == len(lens) and np.isinf(want["value"]).sum() >= 50


def dedup_max_small(api):
    """hnh_tuples_dedup_max: one tuple, all unique, all equal, the maximum first / in the middle / last in its run, equal values inside a
    run, a run that ends at n - 1, a single tuple after a run, nothing at all; and what it refuses.  (Signed zeros: see
    dedup_max_beyond_cap.)"""
    lib, h = api.lib, api.h
    rng = np.random.default_rng(22)
    one = np.ones(1, dtype=bool)
    check_dedup(api, runs_to_tuples(one, np.array([-3.5])), "n = 1")
    check_dedup(api, runs_to_tuples(np.ones(1000, dtype=bool), rng.uniform(-1, 1, 1000)), "all unique")
    eq = np.zeros(1000, dtype=bool); eq[0] = True
    want = check_dedup(api, runs_to_tuples(eq, rng.uniform(-1, 1, 1000)), "all equal")
    assert len(want) == 1
    heads = np.tile([True, False, False, False, False], 5)
    v = np.full(25, -0.5) + np.arange(25) * 1e-3
    for run, at in enumerate((0, 2, 4, 0, 4)):
        v[5 * run + at] = 0.75 + run
    want = check_dedup(api, runs_to_tuples(heads, v), "maximum first, middle, last; the last run ends at n - 1")
    assert np.array_equal(want["value"], 0.75 + np.arange(5))
    v = np.array([0.5, 0.5, 0.25, 0.25, 0.5, 0.5, -1.0, -1.0, -1.0, 2.0])
    heads = np.array([1, 0, 0, 1, 0, 0, 1, 0, 0, 1], dtype=bool)
    want = check_dedup(api, runs_to_tuples(heads, v), "equal values inside a run; a single tuple last")
    assert np.array_equal(want["value"], [0.5, 0.5, -1.0, 2.0])
    check_dedup(api, runs_to_tuples(np.zeros(0, dtype=bool), np.zeros(0)), "n = 0")   # null pointer accepted
    d = api.upload(runs_to_tuples(one, np.array([1.0])))
    cnt = C.c_int64(-1)
    assert lib.hnh_tuples_dedup_max(h, d.ptr, 1, None, 0) != 0       # nowhere to put the count
    assert lib.hnh_tuples_dedup_max(h, d.ptr, -1, C.byref(cnt), 0) != 0
    d.free()


# ---- 2. take_strided
def take_strided(api):
    """hnh_tuples_take_strided: a rank's slice src[first::stride] of CAP + 257 tuples (stride 1: the output is beyond the cap as well);
    the tuples behind the output are not written."""
    lib, h = api.lib, api.h
    src = make_tuples(BIG, 1000, 777, 23)
    d = api.upload(src)
    guard = tuples_of([7, 8], [9, 10], [-1.5, -2.5])
    for first, stride in ((0, 1), (2, 3), (6, 7)):
        n_out = -(-(BIG - first) // stride)
        want = src[first::stride]
        assert len(want) == n_out
        out = api.upload(np.concatenate([np.zeros(n_out, dtype=K.TUPLE_DTYPE), guard]))
        api.check(lib.hnh_tuples_take_strided(h, d.ptr, first, stride, out.ptr, n_out, 0), "take_strided")
        got = fetch(out)
        assert same_bytes(got[:n_out], want) and same_bytes(got[n_out:], guard), (first, stride)
        out.free()
    api.check(lib.hnh_tuples_take_strided(h, d.ptr, 5, 2, None, 0, 0), "take_strided of nothing")
    out = api.upload(guard)
    assert lib.hnh_tuples_take_strided(h, d.ptr, 0, 0, out.ptr, 2, 0) != 0    # stride 0
    assert lib.hnh_tuples_take_strided(h, d.ptr, -1, 1, out.ptr, 2, 0) != 0   # first < 0
    assert same_bytes(fetch(out), guard)
    d.free(); out.free()


# ---- 3. sort
def check_sort(api, t, key, bits, want_key, what):
    """Sorts a copy of t on the backend and compares with the stable argsort of the full 64-bit key, bit for bit (values carried along)."""
    d = api.upload(t)
    api.check(api.lib.hnh_tuples_sort(api.h, d.ptr, len(t), C.byref(key), bits, 0), "tuples_sort " + what)
    want = t[np.argsort(want_key, kind="stable")]
    assert same_bytes(fetch(d), want), what
    d.free()
    return want


def sort_minimal_key_bits(api):
    """hnh_tuples_sort with the FEWEST key bits the host callers pass (32 + row_bits for KEY_ROW_COL, 32 + col_bits for KEY_COL_ROW; the
    very loop of spmat_local.hpp / er_generator.cpp) at dimensions that are a power of two or next to one, the largest index present.
    The minor index uses all of its 32 bits, and full keys repeat (stability).  One bit too few sorts the largest index as 0 without any
    error — on the HIP backend; the CPU double ignores key_bits."""
    rng = np.random.default_rng(24)
    n = 6000
    for dim in (1, 2, 255, 256, 257, 65536, 65537):
        major = rng.integers(0, dim, n).astype(np.uint64)
        major[17] = dim - 1
        minor = np.where(rng.random(n) < 0.5, rng.choice(np.array([0, 1, 1 << 31, (1 << 32) - 1], dtype=np.uint64), n),
                         rng.integers(0, 1 << 32, n, dtype=np.uint64))
        value = np.arange(n) * 0.25
        bits = 32 + host_key_bits(dim)
        for kind, t in ((K.KEY_ROW_COL, tuples_of(major, minor, value)), (K.KEY_COL_ROW, tuples_of(minor, major, value))):
            k = key_of(t, kind)
            assert len(np.unique(k)) < n and int(k.max()) >> 32 == dim - 1
            check_sort(api, t, tuple_key(kind), bits, k, "dim %d kind %d" % (dim, kind))


def sort_by_owner(api):
    """hnh_tuples_sort by KEY_OWNER with owner_bits as SpmatLocal::redistribute computes it, for 1, 3 and 8 owners, every id in the table
    (p - 1 too), both orientations, blocks that do not divide the dimensions (1000 rows in blocks of 111, 777 columns in blocks of 100)."""
    t = make_tuples(20000, 1000, 777, 25)
    t["r"][0], t["c"][0], t["r"][1], t["c"][1] = 999, 776, 0, 0
    for p in (1, 3, 8):
        table = np.random.default_rng(26 + p).permutation(np.arange(80) % p).astype(np.int32)   # 10 x 8 blocks, or 8 x 10 transposed
        assert set(table.tolist()) == set(range(p))
        dtab = api.upload(table)
        for kw in (dict(transpose=0, rib=111, cib=100, ncb=8, table=table), dict(transpose=1, rib=100, cib=111, ncb=10, table=table)):
            k = key_of(t, K.KEY_OWNER, **kw)
            assert int(k.max()) == p - 1
            key = tuple_key(K.KEY_OWNER, kw["transpose"], kw["rib"], kw["cib"], kw["ncb"], dtab.ptr)
            check_sort(api, t, key, host_owner_bits(p), k, "p %d transpose %d" % (p, kw["transpose"]))
        dtab.free()


def sort_is_stable(api):
    """hnh_tuples_sort: equal keys keep their order — all keys equal (nothing moves), and two distinct keys on CAP + 257 tuples (the
    key, index and gather kernels beyond the cap), the values carried along."""
    n = 5000
    t = tuples_of(np.full(n, 41), np.full(n, 1 << 31), np.arange(n) * 0.5)
    for kind in (K.KEY_ROW_COL, K.KEY_COL_ROW):
        check_sort(api, t, tuple_key(kind), 64, key_of(t, kind), "all keys equal")
    rng = np.random.default_rng(27)
    t = tuples_of(rng.integers(0, 2, BIG), np.full(BIG, 5), np.arange(BIG, dtype=np.float64))
    want = check_sort(api, t, tuple_key(K.KEY_ROW_COL), 32 + host_key_bits(2), key_of(t, K.KEY_ROW_COL), "two keys beyond the cap")
    zeros = int(np.count_nonzero(t["r"] == 0))
    assert 0 < zeros < BIG and np.all(np.diff(want["value"][:zeros]) > 0) and np.all(np.diff(want["value"][zeros:]) > 0)


def sort_extremes(api):
    """hnh_tuples_sort with indices 0, 2^31 - 1, 2^31 and 2^32 - 1 under both 32 | 32 keys; key_bits 64, and 0 and 65, which by the
    header mean 64."""
    ext = np.array([0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1], dtype=np.uint64)
    rng = np.random.default_rng(28)
    r, c = np.tile(np.repeat(ext, 4), 8), np.tile(np.tile(ext, 4), 8)
    perm = rng.permutation(len(r))
    t = tuples_of(r[perm], c[perm], np.arange(len(r)) * 1.5)
    for kind in (K.KEY_ROW_COL, K.KEY_COL_ROW):
        for bits in (64, 0, 65):
            check_sort(api, t, tuple_key(kind), bits, key_of(t, kind), "extremes, kind %d, key_bits %d" % (kind, bits))


def sort_col_div_and_tiny(api):
    """hnh_tuples_sort by KEY_COL_DIV with div = 1 (the key is the column) and with div above every column (one bucket: nothing
    moves); one tuple and two tuples."""
    t = make_tuples(20000, 1000, 777, 29)
    t["c"][5] = 776
    check_sort(api, t, tuple_key(K.KEY_COL_DIV, div=1), host_key_bits(777), key_of(t, K.KEY_COL_DIV, div=1), "div = 1")
    k = key_of(t, K.KEY_COL_DIV, div=778)
    assert not k.any()
    check_sort(api, t, tuple_key(K.KEY_COL_DIV, div=778), 1, k, "one bucket")
    for t in (tuples_of([9], [4], [0.5]), tuples_of([9, 3], [4, 8], [0.5, 0.25]), tuples_of([3, 3], [4, 4], [0.5, 0.25]),
              tuples_of([3, 3], [8, 4], [0.5, 0.25])):
        for kind in (K.KEY_ROW_COL, K.KEY_COL_ROW):
            check_sort(api, t, tuple_key(kind), 32 + host_key_bits(10), key_of(t, kind), "n = %d" % len(t))


# ---- 4. bucket_starts
def bucket_starts(api):
    """hnh_tuples_bucket_starts on 200 000 tuples ordered by column (KEY_COL_DIV, div = 1) over 70 000 columns, the first 300 and some
    in between without a tuple: no bucket, one, a workgroup's worth and one more or less, as many as there are keys and one more or
    less, and far more (several workgroups; buckets empty at both ends; starts[nbuckets] < n and = n)."""
    lib, h = api.lib, api.h
    n, ncols = 200000, 70000
    t = make_tuples(n, 1000, ncols - 300, 30)
    t["c"] += np.uint64(300)
    t["c"][0] = ncols - 1
    key = tuple_key(K.KEY_COL_DIV, div=1)
    t = t[np.argsort(t["c"], kind="stable")]
    keys = key_of(t, K.KEY_COL_DIV, div=1)
    assert int(keys.min()) == 300 and int(keys.max()) == ncols - 1 and len(np.unique(keys)) < ncols - 300
    d = api.upload(t)
    for nb in (0, 1, 255, 256, 257, 69999, 70000, 70001, 100000):
        starts = np.full(nb + 2, -7, dtype=np.int64)
        api.check(lib.hnh_tuples_bucket_starts(h, d.ptr, n, C.byref(key), nb, starts.ctypes.data_as(C.c_void_p), 0), "bucket_starts")
        want = np.searchsorted(keys, np.arange(nb + 1, dtype=np.uint64), side="left")
        assert np.array_equal(starts[:nb + 1], want) and starts[nb + 1] == -7, nb
        assert (starts[nb] < n) == (nb < ncols)
    starts = np.full(302, -7, dtype=np.int64)
    api.check(lib.hnh_tuples_bucket_starts(h, None, 0, C.byref(key), 300, starts.ctypes.data_as(C.c_void_p), 0), "bucket_starts of nothing")
    assert not starts[:301].any() and starts[301] == -7
    d.free()


# ---- 5. to_csr
def check_to_csr(api, t, rows, cols, what, want_max=True):
    lib, h = api.lib, api.h
    n = len(t)
    d = api.upload(t) if n else None
    drp = api.upload(np.full(rows + 2, -7, np.int32))                       # one word beyond rowptr's rows + 1
    dci, dv = api.upload(np.full(n + 1, -7, np.int32)), api.upload(np.full(n + 1, -7.0))
    mx = C.c_int(-1)
    api.check(lib.hnh_tuples_to_csr(h, d.ptr if d else None, n, rows, cols, drp.ptr, dci.ptr if n else None, dv.ptr if n else None,
                                    C.byref(mx) if want_max else None, 0), "to_csr " + what)
    want_rp = np.searchsorted(t["r"], np.arange(rows + 1, dtype=np.uint64), side="left").astype(np.int32)
    rp, ci, v = drp.get().reshape(-1), dci.get().reshape(-1), dv.get().reshape(-1)
    assert np.array_equal(rp[:rows + 1], want_rp) and rp[rows + 1] == -7, what
    assert np.array_equal(ci[:n], t["c"].astype(np.int32)) and ci[n] == -7, what
    assert np.array_equal(v[:n].view(np.uint64), t["value"].view(np.uint64)) and v[n] == -7.0, what
    if want_max:
        assert mx.value == int(np.diff(want_rp).max(initial=0)), what
    for x in (d, drp, dci, dv):
        if x:
            x.free()


def to_csr_shapes(api):
    """hnh_tuples_to_csr with rows + 1 below, on and above a workgroup (and one row, and 1000): an empty first row, an empty last row,
    every nonzero in the last row, every nonzero in row 0, a hub row between empty ones; nothing at all on 257 rows; no place for the
    longest row; and a block too wide for 32-bit column indices, which is refused."""
    lib, h = api.lib, api.h
    rng = np.random.default_rng(31)
    cols = 64
    for rows in (1, 255, 256, 257, 1000):
        for pattern in ("empty first row", "empty last row", "all in the last row", "all in row 0", "hub between empty rows"):
            deg = rng.integers(0, 5, rows)
            if pattern == "empty first row":
                deg[0] = 0
            elif pattern == "empty last row":
                deg[rows - 1] = 0
            elif pattern == "all in the last row":
                deg[:] = 0; deg[rows - 1] = 40
            elif pattern == "all in row 0":
                deg[:] = 0; deg[0] = 40
            else:
                hub = rows // 2
                deg[max(hub - 1, 0):hub + 2] = 0; deg[hub] = cols
            rank = rng.random((rows, cols)).argsort(axis=1).argsort(axis=1)
            r, c = np.nonzero(rank < deg[:, None])                      # (row, col) order, distinct columns in a row
            assert len(r) == deg.sum()
            check_to_csr(api, tuples_of(r, c, rng.uniform(-1, 1, len(r))), rows, cols, "%d rows, %s" % (rows, pattern))
    none = np.zeros(0, dtype=K.TUPLE_DTYPE)
    check_to_csr(api, none, 257, cols, "nothing on 257 rows")
    r, c = np.nonzero(rng.random((40, cols)) < 0.3)
    t = tuples_of(r, c, rng.uniform(-1, 1, len(r)))
    check_to_csr(api, t, 40, cols, "max_row_nnz_host = NULL", want_max=False)
    # column indices are stored as int32: a block of more than 2^31 - 1 columns is refused before anything is written
    d, drp, dci, dv = api.upload(t), api.upload(np.full(41, -7, np.int32)), api.upload(np.full(len(t), -7, np.int32)), api.upload(np.full(len(t), -7.0))
    mx = C.c_int(-1)
    for wide in (1 << 31, 1 << 40):
        assert lib.hnh_tuples_to_csr(h, d.ptr, len(t), 40, wide, drp.ptr, dci.ptr, dv.ptr, C.byref(mx), 0) == K.ERR_UNSUPPORTED
    assert np.all(drp.get() == -7) and np.all(dci.get() == -7) and np.all(dv.get() == -7.0) and mx.value == -1
    api.check(lib.hnh_tuples_to_csr(h, d.ptr, len(t), 40, (1 << 31) - 1, drp.ptr, dci.ptr, dv.ptr, C.byref(mx), 0), "to_csr, 2^31 - 1 columns")
    assert np.array_equal(dci.get().reshape(-1), t["c"].astype(np.int32))
    for x in (d, drp, dci, dv):
        x.free()


def to_csr_beyond_cap(api):
    """hnh_tuples_to_csr on CAP + 257 tuples over 70 001 rows (rows + 1 = 273 workgroups and two threads), first and last row occupied"""
    rng = np.random.default_rng(32)
    rows = 70001
    r = np.sort(rng.integers(0, rows, BIG))
    r[0], r[-1] = 0, rows - 1
    first = np.searchsorted(r, r, side="left")
    c = np.arange(BIG) - first                                            # position in the row: increasing inside a row
    check_to_csr(api, tuples_of(r, c, rng.uniform(-1, 1, BIG)), rows, int(c.max()) + 1, "beyond the cap")


# ---- 6. the streaming kernels
def streaming_beyond_cap(api):
    """hnh_tuples_transform, _remap_cols, _relabel and _from_keys on CAP + 257 elements, each against its numpy line: remap_cols with a
    tuple in segment ndest - 1 and a destination of 0, relabel with different tables for rows and columns."""
    lib, h = api.lib, api.h
    n, rows, cols = BIG, 1000, 777
    t0 = make_tuples(n, rows, cols, 33)
    r0, c0 = t0["r"].copy(), t0["c"].copy()
    d = api.upload(t0)
    api.check(lib.hnh_tuples_transform(h, d.ptr, n, 1, 13, 7, 0), "transform")
    assert same_bytes(fetch(d), tuples_of(c0 % np.uint64(13), r0 % np.uint64(7), t0["value"]))
    div, sub, nsub = 100, 34, 3
    dest = np.random.default_rng(34).permutation(8 * nsub).astype(np.int64) * 1000
    seg = (c0 // np.uint64(div)) * np.uint64(nsub) + (c0 % np.uint64(div)) // np.uint64(sub)
    assert int(seg.max()) == len(dest) - 1 and np.any(dest[seg.astype(np.int64)] == 0)
    d.free(); d = api.upload(t0)
    api.check(lib.hnh_tuples_remap_cols(h, d.ptr, n, div, sub, nsub, dest.ctypes.data_as(C.c_void_p), len(dest), 0), "remap_cols")
    want_c = dest[seg.astype(np.int64)].astype(np.uint64) + (c0 % np.uint64(div)) % np.uint64(sub)
    assert same_bytes(fetch(d), tuples_of(r0, want_c, t0["value"]))
    rl = np.random.default_rng(35).permutation(rows).astype(np.uint64) + np.uint64(1 << 33)
    cl = np.random.default_rng(36).permutation(cols).astype(np.uint64) * np.uint64(3)
    drl, dcl = api.upload(rl), api.upload(cl)
    d.free(); d = api.upload(t0)
    api.check(lib.hnh_tuples_relabel(h, d.ptr, n, drl.ptr, dcl.ptr, 0), "relabel")
    assert same_bytes(fetch(d), tuples_of(rl[r0.astype(np.int64)], cl[c0.astype(np.int64)], t0["value"]))
    for x in (d, drl, dcl):
        x.free()
    keys = np.random.default_rng(37).integers(0, 70001 * 65537, n, dtype=np.uint64)
    dk, dt = api.upload(keys), api.upload(np.zeros(n, dtype=K.TUPLE_DTYPE))
    api.check(lib.hnh_tuples_from_keys(h, dk.ptr, 65537, 0, 1, -2.5, dt.ptr, n, 0), "from_keys")
    assert same_bytes(fetch(dt), tuples_of(keys // np.uint64(65537), keys % np.uint64(65537), np.full(n, -2.5)))
    dk.free(); dt.free()


# ---- 7. the generators
ER_CASES = ((70001, 65537, 3000, 7), (3, 3, 1000, 1), (1, 1, 10, 2), (4096, 1 << 20, 5000, 3), (300, 170, 1, 9), (4096, 4096, BIG, 11))
RMAT_CASES = ((1, 50, (0.25, 0.25, 0.25), 1), (20, 300, (0.57, 0.19, 0.19), 1), (8, 2000, (1.0, 0.0, 0.0), 0), (8, 2000, (0.5, 0.25, 0.25), 1),
              (31, 200, (0.57, 0.19, 0.19), 1), (12, BIG, (0.57, 0.19, 0.19), 1))


def generate_er(api, m, n, draws, seed):
    """(sorted unique keys of hnh_generate_er_keys, the device array that holds them): checked against oracle.erdos_renyi_mn"""
    from oracle import oracle as O
    rows, cols = O.erdos_renyi_mn(m, n, draws, seed)
    dk = api.upload(np.full(draws, 0xABCD, dtype=np.uint64))
    cnt = C.c_int64(-1)
    api.check(api.lib.hnh_generate_er_keys(api.h, m, n, draws, seed, dk.ptr, C.byref(cnt), 0), "generate_er_keys")
    want = rows.astype(np.uint64) * np.uint64(n) + cols.astype(np.uint64)
    assert cnt.value == len(want), (m, n, draws, seed, cnt.value, len(want))
    assert np.array_equal(dk.get().reshape(-1)[:cnt.value], want), (m, n, draws, seed)
    return want, dk


def generators_er(api):
    """hnh_generate_er_keys against oracle.erdos_renyi_mn, keys and counts bit for bit: keys above 2^32, nothing but duplicates, a 1 x 1
    grid, m n = 2^32 exactly (the edge of the generator's key-bits loop), a single draw, CAP + 257 draws, no draw; what it refuses; and
    hnh_tuples_from_keys on the keys above 2^32 with 65 537 columns for one rank and for two of three."""
    lib, h = api.lib, api.h
    for case in ER_CASES:
        keys, dk = generate_er(api, *case)
        if case[0] == 70001:
            assert int(keys.max()) >> 32 and len(keys) == case[2]
            for rank, p in ((0, 1), (1, 3), (2, 3)):
                mine = keys[rank::p]
                dt = api.upload(np.zeros(len(mine), dtype=K.TUPLE_DTYPE))
                api.check(lib.hnh_tuples_from_keys(h, dk.ptr, 65537, rank, p, 1.0, dt.ptr, len(mine), 0), "from_keys")
                assert same_bytes(fetch(dt), tuples_of(mine // np.uint64(65537), mine % np.uint64(65537), np.ones(len(mine))))
                dt.free()
        if case[:2] == (3, 3):
            assert len(keys) == 9
        if case[:2] == (1, 1):
            assert len(keys) == 1
        dk.free()
    cnt = C.c_int64(-1)
    api.check(lib.hnh_generate_er_keys(h, 300, 170, 0, 1, None, C.byref(cnt), 0), "generate_er_keys without draws")
    assert cnt.value == 0
    dk = api.upload(np.zeros(4, dtype=np.uint64))
    assert lib.hnh_generate_er_keys(h, 0, 170, 4, 1, dk.ptr, C.byref(cnt), 0) != 0               # no rows
    assert lib.hnh_generate_er_keys(h, 1 << 33, 1 << 33, 4, 1, dk.ptr, C.byref(cnt), 0) != 0     # m n overflows 64 bits
    dk.free()


def generators_rmat(api):
    """hnh_generate_rmat_keys against oracle.rmat, keys and counts bit for bit: one level and 31 levels, a = 1 (the single key 0),
    a + b + c = 1 exactly, 40-bit keys, CAP + 257 edges; what it refuses."""
    from oracle import oracle as O
    lib, h = api.lib, api.h
    for logm, edges, abc, scramble in RMAT_CASES:
        rows, cols = O.rmat(logm, edges, *abc, seed=5, scramble=bool(scramble))
        dk = api.upload(np.full(edges, 0xABCD, dtype=np.uint64))
        cnt = C.c_int64(-1)
        api.check(lib.hnh_generate_rmat_keys(h, logm, edges, abc[0], abc[1], abc[2], 5, scramble, dk.ptr, C.byref(cnt), 0), "generate_rmat_keys")
        want = rows.astype(np.uint64) * np.uint64(1 << logm) + cols.astype(np.uint64)
        assert cnt.value == len(want), (logm, edges, abc, cnt.value, len(want))
        assert np.array_equal(dk.get().reshape(-1)[:cnt.value], want), (logm, edges, abc)
        if logm == 1:
            assert len(want) == 4
        if abc[0] == 1.0:
            assert np.array_equal(want, [0])
        dk.free()
    cnt = C.c_int64(-1)
    dk = api.upload(np.zeros(4, dtype=np.uint64))
    for logm, abc in ((0, (0.25, 0.25, 0.25)), (32, (0.25, 0.25, 0.25)), (8, (-0.1, 0.5, 0.5)), (8, (0.5, -0.1, 0.5)), (8, (0.5, 0.5, -0.1))):
        assert lib.hnh_generate_rmat_keys(h, logm, 4, abc[0], abc[1], abc[2], 5, 1, dk.ptr, C.byref(cnt), 0) != 0, (logm, abc)
    dk.free()


EDGE_BODIES = (dedup_max_beyond_cap, dedup_max_small, take_strided, sort_minimal_key_bits, sort_by_owner, sort_is_stable, sort_extremes,
               sort_col_div_and_tiny, bucket_starts, to_csr_shapes, to_csr_beyond_cap, streaming_beyond_cap, generators_er, generators_rmat)
