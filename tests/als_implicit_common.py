"""Shared body of the implicit-feedback ALS operator tests: api.ImplicitALS on a 15d_fusion2 operator against the numpy definition in
tests/als_implicit_ref.py.  test_als_implicit_cpu.py runs it on the second CPU test double (composed mode, under the stream-order checker),
test_als_implicit_gpu.py on the HIP library in both modes."""
import numpy as np

import als_implicit_ref as IR
import hnh_testlib as T
from distributed_sddmm_amd import api as H

ALG = "15d_fusion2"
STEPS, ITERS = 2, 2


def keyed(world, d, case, subA, subB, values):
    """`values` (one per stored pair, in the case's order) in the like_S_values and the like_ST_values layouts, through the coordinate probe"""
    n = case["N"]
    lookup = dict(zip((case["rows"] * n + case["cols"]).tolist(), values.tolist()))
    A, B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
    out = []
    for mode, like in ((H.K_SDDMM_A, d.like_S_values), (H.K_SDDMM_B, d.like_ST_values)):
        A.upload(T.probe_local(subA, A.shape, True, n)); B.upload(T.probe_local(subB, B.shape, False, n))
        ones, res = like(1.0), like(0.0)
        d.initial_shift(A, B, mode)
        (d.sddmmA if mode == H.K_SDDMM_A else d.sddmmB)(A, B, ones, res)
        keys = np.rint(res.download()).astype(np.int64)
        res.upload(np.array([lookup[k] for k in keys.tolist()], dtype=np.float64))
        out.append(res); ones.free()
    A.free(); B.free()
    return out


class Solver:
    def __init__(self, world, c, case, folded, alg=ALG, lam=IR.LAMBDA):
        self.case = case
        self.sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], case["vals"])
        self.d = d = H.DistributedSparse(world, alg, self.sp, case["R"], c)
        self.subA, self.subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
        self.A, self.B = d.like_A_matrix(0.0), d.like_B_matrix(0.0)
        self.ws = []
        self.als = H.ImplicitALS(d, lam)
        self.ws = keyed(world, d, case, self.subA, self.subB, case["w"])
        self.als.set_confidence(self.ws[0], self.ws[1])
        self.als.set_folded(folded)

    def set(self, a, b):
        self.A.upload(T.fill_local(self.subA, self.A.shape, a)); self.B.upload(T.fill_local(self.subB, self.B.shape, b))
        self.als.set_embeddings(self.A, self.B)

    def get(self):
        self.als.get_embeddings(self.A, self.B)
        return self.A.download(), self.B.download()

    def free(self):
        self.als.free()
        for x in [self.A, self.B] + self.ws:
            x.free()
        self.d.free(); self.sp.free()


def rank_run(world, c, case, folded, steps=STEPS, iters=ITERS):
    s = Solver(world, c, case, folded)
    s.set(case["A"], case["B"])
    losses = [s.als.loss()]
    for _ in range(steps):
        for which in (H.AMAT, H.BMAT):
            s.als.half_step(which, iters)
            losses.append(s.als.loss())
    a, b = s.get()
    out = dict(subA=s.subA, subB=s.subB, A=a, B=b, losses=np.array(losses), gramA=s.als.gram(H.AMAT), gramB=s.als.gram(H.BMAT))
    s.free()
    return out


def run_case(g, R, p, c, folded):
    """One case on the loaded backend, held to the model at T.TOL; returns the assembled factors, Gram matrices and losses."""
    return run_inputs(IR.inputs(g, R), IR.expected(g, R), p, c, folded, g)[0]


def run_inputs(case, want, p, c, folded, g=None):
    """run_case on given inputs and their expected results (tests/gram_cases.py varies the weights and the factors): returns (the
    assembled results, every rank's own with its whole local blocks)."""
    g, R = g or case["name"], case["R"]
    assert T.valid_config(ALG, p, c, R)
    per_rank = H.run_spmd(p, lambda w: rank_run(w, c, case, folded))
    got = dict(A=T.assemble_dense(per_rank, "A", "subA", case["M"], R), B=T.assemble_dense(per_rank, "B", "subB", case["N"], R),
               losses=per_rank[0]["losses"], gramA=per_rank[0]["gramA"], gramB=per_rank[0]["gramB"])
    errs = {k: T.rel(got[k], want[k]) for k in ("A", "B", "gramA", "gramB", "losses")}
    print("als_implicit %s R=%d p=%d c=%d %s: %s" % (g, R, p, c, "folded" if folded else "composed", " ".join("%s=%.2e" % kv for kv in errs.items())))
    assert len(got["losses"]) == 1 + 2 * STEPS
    for o in per_rank:  # every rank reports the same (all-reduced) losses and Gram matrices
        assert T.rel(o["losses"], per_rank[0]["losses"]) <= 1e-15
        assert T.rel(o["gramA"], per_rank[0]["gramA"]) <= 1e-15 and T.rel(o["gramB"], per_rank[0]["gramB"]) <= 1e-15
    for name, e in errs.items():
        assert e <= T.TOL, (g, R, p, c, folded, name, e)
    return got, per_rank
