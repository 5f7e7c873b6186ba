"""Shared test harness: drives the operator API exactly the way oracle/ref_driver.cpp drives the reference
(coordinate-probe SDDMM to key the value slots, global dense fills through a/bSubmatrices, the six
operations each bracketed by initial_shift / de_shift) and assembles per-rank results into global ones."""
from __future__ import annotations

import json
import os

import numpy as np

from distributed_sddmm_amd import api as H
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORACLE_BACKEND = os.path.join(ROOT, "oracle", "liboracle_backend.so")
# the same double with the GAT's optional groups (oracle/hnh_oracle_gat_groups.h): backward, softmax attention, fused backward, training
ORACLE_GAT_BACKEND = os.path.join(ROOT, "oracle", "liboracle_backend_gat.so")
TOL = 1e-11  # fp64, summation order only

DENSE_OUT = ("spmmA", "spmmB", "fusedA", "fusedB")
SPARSE_OUT = ("sddmmA", "sddmmB", "fusedA_buf", "fusedB_buf")


def golden_cases():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def case_inputs(name: str):
    """Regenerates the seeded inputs of a golden case (same recipe as tests/golden/make_golden.py)."""
    meta = golden_cases()[name]
    m, n, r, seed = meta["M"], meta["N"], meta["R"], meta["seed"]
    rows, cols = O.erdos_renyi_mn(m, n, meta["draws"], seed)
    assert len(rows) == meta["nnz"]
    vals = O.sparse_values(rows, cols, n, seed + 1)
    return dict(name=name, M=m, N=n, R=r, rows=rows, cols=cols, vals=vals, A=O.dense_fill(m, r, seed + 2), B=O.dense_fill(n, r, seed + 3))


def golden_outputs(name: str):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def rel(x, y):
    x, y = np.asarray(x), np.asarray(y)
    if x.size == 0:
        return 0.0
    return float(np.max(np.abs(x - y)) / max(float(np.max(np.abs(y))), 1e-300))


def valid_config(alg: str, p: int, c: int, r: int, square: bool = True) -> bool:
    if p % c:
        return False
    if alg.startswith("25d"):
        s = int(round((p // c) ** 0.5))
        if s * s * c != p:
            return False
        return r % (s * (c if alg == "25d_sparse_replicate" else 1)) == 0
    if alg == "15d_sparse":
        return r % (p // c) == 0
    return True


def fill_local(subs: np.ndarray, shape, glob: np.ndarray) -> np.ndarray:
    loc = np.zeros(shape)
    flat, off = loc.reshape(-1), 0
    for top, left, rc, cc in subs:
        blk = np.zeros((rc, cc))
        keep = max(0, min(rc, glob.shape[0] - top))
        blk[:keep] = glob[top:top + keep, left:left + cc]
        flat[off:off + rc * cc] = blk.reshape(-1)
        off += rc * cc
    return loc


def probe_local(subs: np.ndarray, shape, is_a: bool, n: int) -> np.ndarray:
    """A[i,:] = (i, 1, 0..), B[j,:] = (N, j, 0..)  =>  <A[i], B[j]> = i*N + j."""
    loc = np.zeros(shape)
    flat, off = loc.reshape(-1), 0
    for top, left, rc, cc in subs:
        blk = np.zeros((rc, cc))
        gr = np.arange(top, top + rc, dtype=np.float64)
        for j in range(cc):
            gc = left + j
            if is_a:
                blk[:, j] = gr if gc == 0 else (1.0 if gc == 1 else 0.0)
            else:
                blk[:, j] = float(n) if gc == 0 else (gr if gc == 1 else 0.0)
        flat[off:off + rc * cc] = blk.reshape(-1)
        off += rc * cc
    return loc


def run_all_ops(world: H.World, alg: str, c: int, case: dict, make_spmat=None) -> dict:
    """Executes on ONE rank; returns this rank's share of every result.  make_spmat(world) may supply the input matrix (a
    file reader, ...) instead of the case's tuples."""
    sp = make_spmat(world) if make_spmat else H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], case["vals"])
    d = H.DistributedSparse(world, alg, sp, case["R"], c)
    info = d.info()
    subA, subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
    A, B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
    shapeA, shapeB = A.shape, B.shape
    n = case["N"]
    lookup = dict(zip((case["rows"] * n + case["cols"]).tolist(), case["vals"].tolist()))

    def probe(mode, like):
        A.upload(probe_local(subA, shapeA, True, n))
        B.upload(probe_local(subB, shapeB, False, n))
        ones, res = like(1.0), like(0.0)
        d.initial_shift(A, B, mode)
        (d.sddmmA if mode == H.K_SDDMM_A else d.sddmmB)(A, B, ones, res)
        keys = np.rint(res.download()).astype(np.int64)
        ones.free(); res.free()
        return keys

    keysS, keysST = probe(H.K_SDDMM_A, d.like_S_values), probe(H.K_SDDMM_B, d.like_ST_values)
    S, ST = d.like_S_values(0.0), d.like_ST_values(0.0)
    S.upload(np.array([lookup[k] for k in keysS.tolist()], dtype=np.float64))
    ST.upload(np.array([lookup[k] for k in keysST.tolist()], dtype=np.float64))

    def refill():
        A.upload(fill_local(subA, shapeA, case["A"]))
        B.upload(fill_local(subB, shapeB, case["B"]))

    out = dict(info=info, subA=subA, subB=subB, keysS=keysS, keysST=keysST)
    res = d.like_S_values(0.0)
    refill(); d.initial_shift(A, B, H.K_SDDMM_A); d.sddmmA(A, B, S, res); d.de_shift(A, B, H.K_SDDMM_A)
    out["sddmmA"] = res.download()
    # inputs must come back unchanged (the moving operand is shifted and has to be home again on return)
    out["A_after_sddmmA"], out["B_after_sddmmA"] = A.download(), B.download()
    out["A_expected"], out["B_expected"] = fill_local(subA, shapeA, case["A"]), fill_local(subB, shapeB, case["B"])
    res.free()
    res = d.like_ST_values(0.0)
    refill(); d.initial_shift(A, B, H.K_SDDMM_B); d.sddmmB(A, B, ST, res); d.de_shift(A, B, H.K_SDDMM_B)
    out["sddmmB"] = res.download(); res.free()
    refill(); d.initial_shift(A, B, H.K_SPMM_A); d.spmmA(A, B, S); d.de_shift(A, B, H.K_SPMM_A)
    out["spmmA"] = A.download()
    refill(); d.initial_shift(A, B, H.K_SPMM_B); d.spmmB(A, B, ST); d.de_shift(A, B, H.K_SPMM_B)
    out["spmmB"] = B.download()
    buf = d.like_S_values(0.0)
    refill(); d.initial_shift(A, B, H.K_SDDMM_A); d.fusedSpMM(A, B, S, buf, H.AMAT); d.de_shift(A, B, H.K_SDDMM_A)
    out["fusedA"], out["fusedA_buf"] = A.download(), buf.download(); buf.free()
    buf = d.like_ST_values(0.0)
    refill(); d.initial_shift(A, B, H.K_SDDMM_B); d.fusedSpMM(A, B, ST, buf, H.BMAT); d.de_shift(A, B, H.K_SDDMM_B)
    out["fusedB"], out["fusedB_buf"] = B.download(), buf.download(); buf.free()
    # scratch.cpp:26-76 fingerprints
    fps = []
    for mode, op in ((H.K_SDDMM_A, "sddmm"), (H.K_SPMM_A, "spmmA"), (H.K_SPMM_B, "spmmB")):
        d.dummyInitialize(A, H.AMAT); d.dummyInitialize(B, H.BMAT)
        d.initial_shift(A, B, mode)
        if op == "sddmm":
            ones, r2 = d.like_S_values(1.0), d.like_S_values(0.0)
            d.sddmmA(A, B, ones, r2); fps.append(float(np.sum(r2.download() ** 2))); ones.free(); r2.free()
        elif op == "spmmA":
            ones = d.like_S_values(1.0); d.spmmA(A, B, ones); fps.append(float(np.sum(A.download() ** 2))); ones.free()
        else:
            ones = d.like_ST_values(1.0); d.spmmB(A, B, ones); fps.append(float(np.sum(B.download() ** 2))); ones.free()
    out["fingerprints"] = np.array(fps)
    out["alg_info"] = d.json_algorithm_info()
    out["perf"] = d.json_perf_statistics()
    out["borrow"] = d.borrow_stats()
    for x in (A, B, S, ST):
        x.free()
    d.free(); sp.free()
    return out


def assemble(per_rank: list, case: dict) -> dict:
    m, n, r = case["M"], case["N"], case["R"]
    glob = {}
    for name, which, nr in (("spmmA", "subA", m), ("fusedA", "subA", m), ("spmmB", "subB", n), ("fusedB", "subB", n)):
        g = np.zeros((nr, r))
        cover = np.zeros((nr, r), dtype=np.int32)
        for o in per_rank:
            flat, off = o[name].reshape(-1), 0
            for top, left, rc, cc in o[which]:
                blk = flat[off:off + rc * cc].reshape(rc, cc)
                off += rc * cc
                keep = max(0, min(rc, nr - top))
                g[top:top + keep, left:left + cc] = blk[:keep]
                cover[top:top + keep, left:left + cc] += 1
        assert np.all(cover == 1), "submatrices of the ranks must partition the dense matrix"
        glob[name] = g
    for name, kn in (("sddmmA", "keysS"), ("sddmmB", "keysST"), ("fusedA_buf", "keysS"), ("fusedB_buf", "keysST")):
        keys = np.concatenate([o[kn] for o in per_rank])
        vals = np.concatenate([o[name] for o in per_rank])
        order = np.argsort(keys, kind="stable")
        glob[name] = (keys[order], vals[order])
    glob["fingerprints"] = np.sum([o["fingerprints"] for o in per_rank], axis=0)
    return glob


def check_against_golden(glob: dict, per_rank: list, case: dict, alg: str, tol: float = TOL):
    gold = golden_outputs(case["name"])
    keys = case["rows"] * case["N"] + case["cols"]
    fusion2 = (alg == "15d_fusion2")
    for name in DENSE_OUT:
        want = gold[name + "_fusion2"] if (fusion2 and name.startswith("fused")) else gold[name]
        assert rel(glob[name], want) <= tol, (alg, name, rel(glob[name], want))
    for name in SPARSE_OUT:
        k, v = glob[name]
        assert np.array_equal(k, keys), (alg, name, "every nonzero must be owned exactly once")
        if fusion2 and name.endswith("_buf"):
            assert np.all(v == 0.0), "local-kernel-fusion fusedSpMM leaves sddmm_buffer untouched, like the reference"
            continue
        assert rel(v, gold[name]) <= tol, (alg, name, rel(v, gold[name]))
    assert rel(glob["fingerprints"], gold["fingerprints"]) <= tol
    for o in per_rank:  # inputs intact after an SDDMM
        assert np.array_equal(o["A_after_sddmmA"], o["A_expected"])
        assert np.array_equal(o["B_after_sddmmA"], o["B_expected"])


def make_case(name, m, n, r, rows, cols, seed=11):
    """A case with hashed S values / dense fills, for inputs that have no golden fixture (checked vs the oracle)."""
    return dict(name=name, M=m, N=n, R=r, rows=rows, cols=cols, vals=O.sparse_values(rows, cols, n, seed),
                A=O.dense_fill(m, r, seed + 1), B=O.dense_fill(n, r, seed + 2))


def check_against_oracle(glob: dict, case: dict, alg: str, tol: float = TOL):
    """Same checks as check_against_golden, against oracle/oracle.py (itself pinned to the reference by
    tests/test_oracle_golden.py) — for sizes / matrices that have no committed fixture."""
    rows, cols, vals, a, b, m, n = case["rows"], case["cols"], case["vals"], case["A"], case["B"], case["M"], case["N"]
    keys = rows * n + cols
    ign = alg == "15d_fusion2"
    want_sddmm = O.sddmm(rows, cols, vals, a, b)
    for name in ("sddmmA", "sddmmB"):
        assert np.array_equal(glob[name][0], keys), (alg, name)
        assert rel(glob[name][1], want_sddmm) <= tol, (alg, name, rel(glob[name][1], want_sddmm))
    assert rel(glob["spmmA"], O.spmm_a(rows, cols, vals, b, m)) <= tol
    assert rel(glob["spmmB"], O.spmm_b(rows, cols, vals, a, n)) <= tol
    fa, mid = O.fused_a(rows, cols, vals, a, b, ign)
    fb, _ = O.fused_b(rows, cols, vals, a, b, ign)
    assert rel(glob["fusedA"], fa) <= tol and rel(glob["fusedB"], fb) <= tol
    if not ign:
        assert rel(glob["fusedA_buf"][1], mid) <= tol and rel(glob["fusedB_buf"][1], mid) <= tol
    assert rel(glob["fingerprints"], np.array(O.fingerprints(rows, cols, m, n, case["R"]))) <= tol


# ALS factors and residuals against the reference's: batched CG amplifies summation-order differences — the reference's OWN five
# schedules disagree by up to 1.14e-11 on the golden cases (tests/golden/als_manifest.json, "deviation_from_canonical") — so the bound is
# 10 x that spread.  What this repository's path actually differs by is recorded in the same manifest ("observed_vs_reference": HIP on
# an MI355X and the CPU test double, fixtures and config 2's full size): at most a few 1e-12.
ALS_TOL = 1.2e-10


def record_observed(kind, **fields):
    """Append one observed-error record to $HNH_OBSERVED_LOG (JSON lines) — how the numbers in als_manifest.json were collected."""
    path = os.environ.get("HNH_OBSERVED_LOG")
    if path:
        import json
        with open(path, "a") as f:
            f.write(json.dumps(dict({"kind": kind, "backend": H.backend_name()}, **{k: (float(v) if isinstance(v, (float, np.floating)) else v) for k, v in fields.items()})) + "\n")


def run_als(world: H.World, alg: str, c: int, case: dict, steps: int, iters: int) -> dict:
    """ALS-CG driven like oracle/ref_driver.cpp's `als` mode: ground truth = the case's S values (keyed through
    the coordinate probe), embeddings from the case's A, B, then `steps` alternating CG solves."""
    sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], case["vals"])
    d = H.DistributedSparse(world, alg, sp, case["R"], c)
    subA, subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
    A, B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
    n = case["N"]
    lookup = dict(zip((case["rows"] * n + case["cols"]).tolist(), case["vals"].tolist()))
    gts = []
    for mode, like in ((H.K_SDDMM_A, d.like_S_values), (H.K_SDDMM_B, d.like_ST_values)):
        A.upload(probe_local(subA, A.shape, True, n)); B.upload(probe_local(subB, B.shape, False, n))
        ones, res = like(1.0), like(0.0)
        d.initial_shift(A, B, mode)
        (d.sddmmA if mode == H.K_SDDMM_A else d.sddmmB)(A, B, ones, res)
        keys = np.rint(res.download()).astype(np.int64)
        res.upload(np.array([lookup[k] for k in keys.tolist()], dtype=np.float64))
        gts.append(res); ones.free()
    als = H.DistributedALS(d, False)
    als.set_ground_truth(gts[0], gts[1])
    A.upload(fill_local(subA, A.shape, case["A"])); B.upload(fill_local(subB, B.shape, case["B"]))
    als.set_embeddings(A, B)
    residuals = [als.computeResidual()]
    for _ in range(steps):
        als.cg_optimizer(H.AMAT, iters)
        als.cg_optimizer(H.BMAT, iters)
        residuals.append(als.computeResidual())
    als.get_embeddings(A, B)
    out = dict(subA=subA, subB=subB, alsA=A.download(), alsB=B.download(), residuals=np.array(residuals))
    als.free()
    for x in (A, B, gts[0], gts[1]):
        x.free()
    d.free(); sp.free()
    return out


def assemble_dense(per_rank, name, which, nrows, r):
    g = np.zeros((nrows, r))
    for o in per_rank:
        flat, off = o[name].reshape(-1), 0
        for top, left, rc, cc in o[which]:
            blk = flat[off:off + rc * cc].reshape(rc, cc)
            off += rc * cc
            keep = max(0, min(rc, nrows - top))
            g[top:top + keep, left:left + cc] = blk[:keep]
    return g


def check_als_against_golden(per_rank, case):
    gold = dict(np.load(os.path.join(GOLDEN, "als_%s.npz" % case["name"])))
    a = assemble_dense(per_rank, "alsA", "subA", case["M"], case["R"])
    b = assemble_dense(per_rank, "alsB", "subB", case["N"], case["R"])
    record_observed("als_fixture", case=case["name"], ranks=len(per_rank), A=rel(a, gold["A"]), B=rel(b, gold["B"]),
                    residuals=rel(per_rank[0]["residuals"], gold["residuals"]))
    assert rel(a, gold["A"]) <= ALS_TOL, rel(a, gold["A"])
    assert rel(b, gold["B"]) <= ALS_TOL, rel(b, gold["B"])
    assert rel(per_rank[0]["residuals"], gold["residuals"]) <= ALS_TOL
    assert gold["residuals"][-1] < 0.2 * gold["residuals"][0], "ALS must reduce the residual"


GAT_LAYERS = [(16, 8, 2), (16, 4, 3)]  # (input_features, features_per_head, num_heads)
GAT_ALPHA = 0.2
GAT_INPUT_SCALE = 50.0


def run_gat(world: H.World, alg: str, c: int, case: dict, layers=None, alpha: float = GAT_ALPHA) -> dict:
    """GAT forward pass driven like oracle/ref_driver.cpp's `gat` mode (same hashed weights, input = case A)."""
    layers = layers or GAT_LAYERS
    sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
    d = H.DistributedSparse(world, alg, sp, case["R"], c)
    gnn = H.GAT(d, layers, alpha)
    for li, (fin, fph, heads) in enumerate(layers):
        for h in range(heads):
            k, n = gnn.weight_shape(li, h)
            gnn.set_weight(li, h, O.gat_weight(li, h, k, n))
    d.setRValue(layers[0][0])
    subB = d.submatrices(H.BMAT)
    x = H.Dense.create(world, *gnn.buffer_shape(0))
    x.upload(fill_local(subB, x.shape, case["A"] * GAT_INPUT_SCALE))
    gnn.set_input(x)
    gnn.forwardPass()
    d.setRValue(layers[-1][1] * layers[-1][2])
    subA = d.submatrices(H.AMAT)
    out = H.Dense.create(world, *gnn.buffer_shape(len(layers)))
    gnn.get_output(out)
    res = dict(subA=subA, gat=out.download())
    x.free(); out.free(); gnn.free(); d.free(); sp.free()
    return res


# ---------------------------------------------------------------------------------------------- fusedSpMM_out
def run_fused_out(world: H.World, alg: str, c: int, case: dict, matmode: int, leaky_alpha, x_scale: float, want_rowdot: bool) -> dict:
    """Distributed_Sparse::fusedSpMM_out on ONE rank; returns this rank's rows of Out / rowdot and the untouched inputs."""
    sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
    d = H.DistributedSparse(world, alg, sp, case["R"], c)
    subA, subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
    A, B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
    A.upload(fill_local(subA, A.shape, case["A"])); B.upload(fill_local(subB, B.shape, case["B"]))
    x = A if matmode == H.AMAT else B
    out = H.Dense.create(world, *x.shape); out.fill(7.0)  # must be overwritten, not accumulated into
    dot = H.Vec.create(world, x.shape[0]) if want_rowdot else None
    ok = d.fusedSpMM_out(A, B, matmode, out, leaky_alpha=leaky_alpha, x_scale=x_scale, rowdot=dot)
    res = dict(supported=ok, subA=subA, subB=subB)
    if ok:
        res.update(out=out.download(), rowdot=dot.download() if dot else None, A_after=A.download(), B_after=B.download(),
                   A_expected=fill_local(subA, A.shape, case["A"]), B_expected=fill_local(subB, B.shape, case["B"]))
    for h in (A, B, out, dot):
        if h is not None:
            h.free()
    d.free(); sp.free()
    return res


def fused_out_expected(case: dict, matmode: int, leaky_alpha, x_scale: float):
    """numpy restatement: w = LeakyReLU(<X_i, Y_j>), Out = sum_e w_e Y_j + x_scale X, rowdot = <X_i, Out_i> (S == 1)."""
    rows, cols = (case["rows"], case["cols"]) if matmode == H.AMAT else (case["cols"], case["rows"])
    X, Y = (case["A"], case["B"]) if matmode == H.AMAT else (case["B"], case["A"])
    w = np.einsum("ij,ij->i", X[rows], Y[cols])
    if leaky_alpha is not None:
        w = np.where(w > 0, w, leaky_alpha * w)
    out = np.zeros_like(X)
    np.add.at(out, rows, w[:, None] * Y[cols])
    out = out + x_scale * X
    return out, np.einsum("ij,ij->i", X, out)


def check_fused_out(per_rank, case, matmode, leaky_alpha, x_scale, want_rowdot):
    which, nrows = ("subA", case["M"]) if matmode == H.AMAT else ("subB", case["N"])
    got = assemble_dense(per_rank, "out", which, nrows, case["R"])
    want, want_dot = fused_out_expected(case, matmode, leaky_alpha, x_scale)
    assert rel(got, want) <= TOL
    for o in per_rank:  # inputs untouched (the moving operand is only read)
        assert np.array_equal(o["A_after"], o["A_expected"]) and np.array_equal(o["B_after"], o["B_expected"])
    if want_rowdot:
        scale = float(np.max(np.abs(want_dot))) or 1.0
        for o in per_rank:  # one entry per local row, rows listed by the submatrix descriptors
            off = 0
            for top, left, rc, cc in o[which]:
                keep = max(0, min(rc, nrows - top))
                if keep > 0:  # a rank whose rows are all padding (M < p * rows per rank) has nothing to compare
                    assert np.max(np.abs(o["rowdot"][off:off + keep] - want_dot[top:top + keep])) <= TOL * scale
                off += rc


def write_symmetric_mtx_with_duplicates(path, n, seed):
    """A symmetric MatrixMarket file (lower triangle stored) in which about a third of the entries appear two or three
    times with different values.  Returns the tuples a reader must produce: both triangles, duplicates merged by MAXIMUM
    (the reference reads with maximum<double>(), SpmatLocal.hpp:485-498)."""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, 6 * n), rng.integers(0, n, 6 * n)
    lo = np.unique(np.maximum(r, c) * n + np.minimum(r, c))           # distinct lower-triangle coordinates
    dup = np.concatenate([lo, lo[::3], lo[::7]])
    rng.shuffle(dup)
    vals = rng.uniform(-1, 1, len(dup))
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n% written by the test\n" + "%d %d %d\n" % (n, n, len(dup)))
        for k, v in zip(dup.tolist(), vals.tolist()):
            f.write("%d %d %.17g\n" % (k // n + 1, k % n + 1, v))
    best = {}
    for k, v in zip(dup.tolist(), vals.tolist()):
        best[k] = max(best.get(k, -np.inf), v)
    rows, cols, out = [], [], []
    for k, v in best.items():
        i, j = k // n, k % n
        rows.append(i); cols.append(j); out.append(v)
        if i != j:
            rows.append(j); cols.append(i); out.append(v)
    rows, cols, out = np.array(rows), np.array(cols), np.array(out)
    order = np.argsort(rows * n + cols)
    return rows[order], cols[order], out[order]
