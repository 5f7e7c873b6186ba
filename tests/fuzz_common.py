"""The generator of the randomised differential tests of the host logic (tests/test_fuzz_cpu.py, and over the RCCL emulation
tests/test_rccl_emulation_cpu.py): one() draws a schedule, a grid, sizes and host switches and checks the run against the numpy oracle;
sweep() does `count` draws from one seed and restores the environment.  `python tests/fuzz_common.py SEED COUNT` explores further."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # stand-alone use: python tests/fuzz_common.py
import hnh_testlib as T  # noqa: E402
from distributed_sddmm_amd import api as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

GRIDS = [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4), (8, 8),
         (3, 1), (3, 3), (5, 1), (6, 2), (6, 3), (7, 1), (9, 1), (9, 3), (12, 2), (12, 3), (16, 4), (18, 2)]  # (grids with remainders)
KNOBS = ("HNH_MESH_CHUNKS", "HNH_RING_MODE", "HNH_HOST_SETUP", "HNH_ACC_HALVES", "HNH_BORROW", "HNH_SHIP_INDICES", "HNH_MESH_TAPER",
         "HNH_WINDOW_MERGE", "HNH_WINDOW_MERGE_CAP", "HNH_ORACLE_EVENTS_PENDING")
# switches that select another host code path: the whole accumulator instead of two halves, borrowed value arrays off / forced,
# the reference's shift payload, chunk heights of the mesh fetch
EXTRA = {"HNH_ACC_HALVES": [None, "0"], "HNH_BORROW": [None, "off", "force"], "HNH_SHIP_INDICES": [None, "1"],
         "HNH_MESH_TAPER": [None, None, "1,2,2,2,1,1", "3,4,4,3,2,1,1", "2,1"],
         # adaptive chunk windows of the mesh fetch: off, at most n chunks per pass, and arrival events that answer "not yet" to every
         # k-th query of the host (the test double completes everything at once: without this every pass would take all chunks)
         "HNH_WINDOW_MERGE": [None, None, "0"], "HNH_WINDOW_MERGE_CAP": [None, "1", "2", "3"], "HNH_ORACLE_EVENTS_PENDING": [None, "2", "3"]}


def one(rng, it):
    alg = rng.choice(H.ALGORITHMS)
    p, c = rng.choice(GRIDS)
    r = rng.choice([4, 8, 12, 16, 24])
    if not T.valid_config(alg, p, c, r):
        return None
    m = rng.choice([5, 9, 17, 40, 64, 100, 130])
    n = m if rng.random() < 0.5 else rng.choice([7, 23, 64, 90, 150])
    draws = rng.choice([1, 10, m * 3, m * 8])
    for k, choices in EXTRA.items():
        v = rng.choice(choices)
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    os.environ["HNH_MESH_CHUNKS"] = str(rng.choice([1, 2, 3, 4, 8]))
    os.environ["HNH_RING_MODE"] = rng.choice(["mesh", "relay"])
    if rng.random() < 0.3:
        os.environ["HNH_HOST_SETUP"] = "1"
    else:
        os.environ.pop("HNH_HOST_SETUP", None)
    rows, cols = O.erdos_renyi_mn(m, n, draws, 1000 + it)
    case = T.make_case("fz%d" % it, m, n, r, rows, cols, seed=it)
    tag = "%s p=%d c=%d R=%d %dx%d nnz=%d %s" % (alg, p, c, r, m, n, len(rows), {k: os.environ.get(k) for k in KNOBS})
    per_rank = H.run_spmd(p, lambda w: T.run_all_ops(w, alg, c, case))
    T.check_against_oracle(T.assemble(per_rank, case), case, alg)
    if alg == "15d_fusion2":
        for mm in (H.AMAT, H.BMAT):
            pr = H.run_spmd(p, lambda w: T.run_fused_out(w, alg, c, case, mm, 0.3, 0.7, True))
            T.check_fused_out(pr, case, mm, 0.3, 0.7, True)
    if len(rows) >= m and rng.random() < 0.5:
        # ALS: the CG iteration folded into the fused call's row epilogue (hnh_cg_update; schedules without an R split) against
        # the variant with the reference's separate update steps — whatever the schedule, grid and route, the same factors
        both = []
        for unfolded in (False, True):
            if unfolded:
                os.environ["HNH_ALS_UNFOLDED"] = "1"
            else:
                os.environ.pop("HNH_ALS_UNFOLDED", None)
            pr = H.run_spmd(p, lambda w: T.run_als(w, alg, c, case, 1, 3))
            both.append((T.assemble_dense(pr, "alsA", "subA", m, r), T.assemble_dense(pr, "alsB", "subB", n, r), pr[0]["residuals"]))
        os.environ.pop("HNH_ALS_UNFOLDED", None)
        for x, y in zip(*both):
            assert T.rel(x, y) <= T.ALS_TOL, tag
        tag += " +als"
    return tag


def sweep(seed, count):
    saved = {k: os.environ.get(k) for k in KNOBS}
    rng = random.Random(seed)
    done = []
    try:
        for it in range(count):
            tag = one(rng, it)
            if tag:
                done.append(tag)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return done


if __name__ == "__main__":
    H.load_backend(T.ORACLE_BACKEND)
    for t in sweep(int(sys.argv[1]) if len(sys.argv) > 1 else 1, int(sys.argv[2]) if len(sys.argv) > 2 else 40):
        print("ok", t)
