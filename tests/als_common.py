"""Shared body of the ALS-CG width / graph / schedule tests: the whole application through the operator API (DistributedALS over every
schedule) against the numpy definition in tests/als_ref.py.  test_als_widths_cpu.py runs it on the oracle's C test double (host logic),
test_als_widths_gpu.py on the HIP library; test_als_model_cpu.py holds the definition itself down and checks, for every case listed
here, that float64 is a good enough model (within ALS_TOL / 10 of long double).

Two ways of driving the solver, because batched CG on these rank-deficient systems amplifies rounding:
  free    3 alternating steps x 1 CG iteration, factors uploaded once — a held operand at an unchanged address with changed contents
          from the third half-step on;
  forced  2 alternating steps x 2 CG iterations, every half-step started from the model's state.
"""
import functools
import json
import os

import numpy as np

import als_ref
import hnh_testlib as T
from distributed_sddmm_amd import api as H
from oracle import oracle as O

FREE = ("free", 3, 1)      # mode, alternating steps, CG iterations
FORCED = ("forced", 2, 2)
MODES = {"free": FREE, "forced": FORCED}

HUB_M, HUB_N = 1100, 2100
LONG_ROW = 256             # kLongRowMin: rows longer than this leave the fused kernel's row pass for the segment path


def _first_of_permutation(n, count, seed):
    """`count` distinct indices below n, picked by the oracle's hashed vertex permutation."""
    return np.flatnonzero(O.vertex_permutation(n, seed) < count)


@functools.lru_cache(maxsize=None)
def graph(name):
    """(M, N, rows, cols), row-major sorted, built from the oracle's generators only."""
    if name == "hub":
        m, n = HUB_M, HUB_N
        rows, cols = O.erdos_renyi_mn(m, n, 8 * m, 77)
        extra = [(np.full(1500, 1), _first_of_permutation(n, 1500, 5)),            # two hub rows of S
                 (np.full(1100, m // 2), _first_of_permutation(n, 1100, 6)),
                 (_first_of_permutation(m, 1050, 7), np.full(1050, 5))]            # a hub row of S^T
        keys = np.unique(np.concatenate([rows * n + cols] + [r * n + c for r, c in extra]))
        keys = keys[(keys // n != 7) & (keys % n != 11)]                           # one row and one column empty for certain
        return m, n, keys // n, keys % n
    if name == "rmat":
        rows, cols = O.rmat(10, 16 * 1024)
        return 1024, 1024, rows, cols
    raise KeyError(name)


def seeds(name, R, mode):
    """Fill seeds (ground truth, A, B) of a case: tests/golden/als_manifest.json "model_condition" lists the ones that were chosen
    to meet the float64-vs-long-double condition; every other case uses the default."""
    return tuple(_manifest()["model_condition"]["seeds"].get("%s R%d %s" % (name, R, mode), _manifest()["model_condition"]["default_seeds"]))


@functools.lru_cache(maxsize=None)
def _manifest():
    with open(os.path.join(T.GOLDEN, "als_manifest.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def inputs(name, R, mode):
    m, n, rows, cols = graph(name)
    sv, sa, sb = seeds(name, R, mode)
    case = dict(name="%s_r%d" % (name, R), M=m, N=n, R=R, rows=rows, cols=cols, vals=O.sparse_values(rows, cols, n, sv),
                A=O.dense_fill(m, R, sa), B=O.dense_fill(n, R, sb))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def expected(name, R, mode):
    """The float64 model's answer, computed once per (graph, R, mode) and shared by every schedule: free -> (A, B, residuals),
    forced -> als_ref.forced()'s list."""
    c = inputs(name, R, mode)
    _, steps, iters = MODES[mode]
    if mode == "free":
        return als_ref.run(c["rows"], c["cols"], c["vals"], c["A"], c["B"], steps, iters, np.float64)
    return als_ref.forced(c["rows"], c["cols"], c["vals"], c["A"], c["B"], steps, iters, np.float64)


# ------------------------------------------------------------------------------------------------ the cases (ISSUE table)
WIDTHS = (2, 8, 17, 32, 100, 128, 130, 256, 257, 384, 600)
FORCED_WIDTHS = tuple(_manifest()["model_condition"]["forced_widths_hub"])   # ends at 384 if R = 600 misses the condition
SCHEDULES = (("15d_fusion2", 4, 2), ("15d_fusion2", 8, 2), ("15d_fusion2", 5, 1), ("15d_fusion1", 4, 1), ("15d_fusion1", 6, 2),
             ("15d_sparse", 4, 1), ("15d_sparse", 8, 2), ("25d_dense_replicate", 4, 1), ("25d_dense_replicate", 8, 2),
             ("25d_sparse_replicate", 8, 2))
SCHEDULE_WIDTHS = (8, 100, 256)
ALL_ALGS = ("15d_fusion2", "15d_fusion1", "15d_sparse", "25d_dense_replicate", "25d_sparse_replicate")
# forced mode at R = 128 on `hub` under each switch: (id, alg, p, c, environment)
VARIANTS = (("no_hold", "15d_fusion2", 4, 1, {"HNH_NO_HOLD": "1"}),
            ("relay", "15d_fusion2", 4, 1, {"HNH_RING_MODE": "relay"}),
            ("unfolded", "15d_fusion2", 4, 1, {"HNH_ALS_UNFOLDED": "1"}),
            ("one_mesh_chunk", "15d_fusion2", 4, 1, {"HNH_MESH_CHUNKS": "1"}),
            ("relay_ring_of_two", "15d_fusion2", 2, 1, {"HNH_RING_MODE": "relay"}))


def gpu_solver_cases():
    """(graph, R, mode, alg, p, c) of rows 1-3 of the table."""
    out = []
    for mode in ("free", "forced"):
        for p in (1, 4):
            out += [("hub", R, mode, "15d_fusion2", p, 1) for R in (WIDTHS if mode == "free" else FORCED_WIDTHS)]
        out += [("rmat", R, mode, "15d_fusion2", 1, 1) for R in (128, 256)]
        out += [("hub", R, mode, alg, p, c) for alg, p, c in SCHEDULES for R in SCHEDULE_WIDTHS]
    return out


def artificial_cases(widths=(8, 100)):
    """(alg, p, c, R) of row 5: every schedule at (4, 1), or (8, 2) where (4, 1) is not a valid grid for it."""
    out = []
    for alg in ALL_ALGS:
        for R in widths:
            p, c = (4, 1) if T.valid_config(alg, 4, 1, R) else (8, 2)
            assert T.valid_config(alg, p, c, R)
            out.append((alg, p, c, R))
    return out


def cpu_solver_cases():
    out = [("hub", R, mode, "15d_fusion2", p, 1) for mode in ("free", "forced") for p in (1, 4) for R in (8, 17, 100, 128, 257)]
    for alg in ALL_ALGS[1:]:
        p, c = (4, 1) if T.valid_config(alg, 4, 1, 8) else (8, 2)
        out += [("hub", 8, mode, alg, p, c) for mode in ("free", "forced")]
    return out


def model_cases():
    """Every (graph, R, mode) an operator test uses, on either backend."""
    seen = []
    for g, R, mode, *_ in gpu_solver_cases() + cpu_solver_cases() + [("hub", 128, "forced")]:
        if (g, R, mode) not in seen:
            seen.append((g, R, mode))
    return seen


def case_id(c):
    return "-".join(str(x) for x in c)


# ------------------------------------------------------------------------------------------------ through the operator
class Solver:
    """One rank's DistributedALS over a case, ground truth keyed through the coordinate probe like T.run_als."""

    def __init__(self, world, alg, c, case):
        self.case = case
        self.sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], case["vals"])
        self.d = d = H.DistributedSparse(world, alg, self.sp, case["R"], c)
        self.subA, self.subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
        self.A, self.B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
        n = case["N"]
        lookup = dict(zip((case["rows"] * n + case["cols"]).tolist(), case["vals"].tolist()))
        self.gts = []
        for mode, like in ((H.K_SDDMM_A, d.like_S_values), (H.K_SDDMM_B, d.like_ST_values)):
            self.A.upload(T.probe_local(self.subA, self.A.shape, True, n)); self.B.upload(T.probe_local(self.subB, self.B.shape, False, n))
            ones, res = like(1.0), like(0.0)
            d.initial_shift(self.A, self.B, mode)
            (d.sddmmA if mode == H.K_SDDMM_A else d.sddmmB)(self.A, self.B, ones, res)
            keys = np.rint(res.download()).astype(np.int64)
            res.upload(np.array([lookup[k] for k in keys.tolist()], dtype=np.float64))
            self.gts.append(res); ones.free()
        self.als = H.DistributedALS(d, False)
        self.als.set_ground_truth(self.gts[0], self.gts[1])

    def set(self, a, b):
        self.A.upload(T.fill_local(self.subA, self.A.shape, a)); self.B.upload(T.fill_local(self.subB, self.B.shape, b))
        self.als.set_embeddings(self.A, self.B)

    def get(self):
        self.als.get_embeddings(self.A, self.B)
        return self.A.download(), self.B.download()

    def free(self):
        self.als.free()
        for x in (self.A, self.B, self.gts[0], self.gts[1]):
            x.free()
        self.d.free(); self.sp.free()


def rank_free(world, alg, c, case, steps, iters):
    s = Solver(world, alg, c, case)
    s.set(case["A"], case["B"])
    residuals = [s.als.computeResidual()]
    for _ in range(steps):
        s.als.cg_optimizer(H.AMAT, iters)
        s.als.cg_optimizer(H.BMAT, iters)
        residuals.append(s.als.computeResidual())
    a, b = s.get()
    out = dict(subA=s.subA, subB=s.subB, alsA=a, alsB=b, residuals=np.array(residuals))
    s.free()
    return out


def rank_forced(world, alg, c, case, states, iters):
    s = Solver(world, alg, c, case)
    out = dict(subA=s.subA, subB=s.subB)
    for k, (which, a_in, b_in, _) in enumerate(states):
        s.set(a_in, b_in)
        s.als.cg_optimizer(H.BMAT if which else H.AMAT, iters)
        a, b = s.get()
        out["half%d" % k] = b if which else a
        out["other%d" % k] = a if which else b
    s.free()
    return out


def assembled(per_rank, name, which, case):
    return T.assemble_dense(per_rank, name, "subB" if which else "subA", case["N"] if which else case["M"], case["R"])


RESULTS = {}   # (graph, R, mode, alg, p, c) -> what the operator returned, for comparisons between cases (hold against no hold)


def run_case(g, R, mode, alg, p, c, tag=""):
    """Runs one case on the loaded backend and holds it to the model at T.ALS_TOL.  Returns the operator's factors."""
    assert T.valid_config(alg, p, c, R), (alg, p, c, R)
    case, want = inputs(g, R, mode), expected(g, R, mode)
    _, steps, iters = MODES[mode]
    if mode == "free":
        per_rank = H.run_spmd(p, lambda w: rank_free(w, alg, c, case, steps, iters))
        got = dict(A=assembled(per_rank, "alsA", 0, case), B=assembled(per_rank, "alsB", 1, case), residuals=per_rank[0]["residuals"])
        errs = dict(A=T.rel(got["A"], want[0]), B=T.rel(got["B"], want[1]), residuals=T.rel(got["residuals"], want[2]))
        assert len(got["residuals"]) == steps + 1
        for o in per_rank:  # every rank reports the same (all-reduced) residuals
            assert T.rel(o["residuals"], per_rank[0]["residuals"]) <= 1e-15
    else:
        per_rank = H.run_spmd(p, lambda w: rank_forced(w, alg, c, case, want, iters))
        got, errs = {}, {}
        for k, (which, a_in, b_in, new) in enumerate(want):
            got[k] = assembled(per_rank, "half%d" % k, which, case)
            errs["half%d" % k] = T.rel(got[k], new)
            # the fixed factor of a half-step comes back as it went in
            assert np.array_equal(assembled(per_rank, "other%d" % k, 1 - which, case), b_in if which == 0 else a_in)
    T.record_observed("als_widths", graph=g, R=R, mode=mode, alg=alg, p=p, c=c, variant=tag, worst=max(errs.values()), **errs)
    print("als_widths %s %s R=%d %s p=%d c=%d %s: %s" % (g, mode, R, alg, p, c, tag, " ".join("%s=%.2e" % kv for kv in errs.items())))
    for name, e in errs.items():
        assert e <= T.ALS_TOL, (g, R, mode, alg, p, c, tag, name, e)
    RESULTS[(g, R, mode, alg, p, c, tag)] = got
    return got


def rank_artificial(world, alg, c, case, seed):
    sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
    d = H.DistributedSparse(world, alg, sp, case["R"], c)
    als = H.DistributedALS(d, True, seed=seed)
    als.initializeEmbeddings()
    A, B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
    als.get_embeddings(A, B)
    out = dict(subA=d.submatrices(H.AMAT), subB=d.submatrices(H.BMAT), alsA=A.download(), alsB=B.download(), residual=als.computeResidual())
    als.free(); A.free(); B.free(); d.free(); sp.free()
    return out


def run_artificial(alg, p, c, R, seed=7):
    """Distributed_ALS(d, true) + initializeEmbeddings: hashed_fill through the schedule's submatrix descriptors (topRow AND leftCol),
    bit for bit against the global hash; the residual against the model's (the ground truth's factors are 1 / (R M R) small, so this
    residual is the embeddings': it shows that the constructor's two SDDMMs ran and gave small numbers, not their digits)."""
    m, n, rows, cols = graph("hub")
    case = dict(M=m, N=n, R=R, rows=rows, cols=cols)
    per_rank = H.run_spmd(p, lambda w: rank_artificial(w, alg, c, case, seed))
    agt, bgt, a0, b0 = als_ref.hashed_init(m, n, R, seed)
    assert np.array_equal(assembled(per_rank, "alsA", 0, case), a0)
    assert np.array_equal(assembled(per_rank, "alsB", 1, case), b0)
    want = als_ref.residual(rows, cols, als_ref.rowdot(agt[rows], bgt[cols]), a0, b0)
    err = max(abs(o["residual"] - want) / want for o in per_rank)
    T.record_observed("als_widths", graph="hub", R=R, mode="artificial", alg=alg, p=p, c=c, variant="", worst=err, residual=err)
    assert err <= T.TOL, (alg, p, c, R, err)
