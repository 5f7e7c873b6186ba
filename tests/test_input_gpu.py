"""The input side of the operator on the HIP backend: a MatrixMarket file with duplicates (sort + hnh_tuples_dedup_max + hnh_tuples_take_strided
on the GPU), generated input (hnh_generate_er_keys / hnh_generate_rmat_keys + hnh_tuples_from_keys + hnh_tuples_relabel), each under the
device set-up and under HNH_HOST_SETUP=1 (the reference's host algorithm restated), and the two set-ups against each other nonzero by
nonzero.  The CPU twins of the first two are in test_configs_cpu.py."""
import numpy as np
import pytest

import hnh_testlib as T
from distributed_sddmm_amd import api as H
from gat_gpu_harness import hip_backend  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def choose_setup(monkeypatch, host_setup):
    if host_setup:
        monkeypatch.setenv("HNH_HOST_SETUP", "1")
    else:
        monkeypatch.delenv("HNH_HOST_SETUP", raising=False)


@pytest.mark.parametrize("host_setup", [False, True])
def test_matrix_market_file_through_the_schedules_hip(tmp_path, monkeypatch, host_setup):
    """A symmetric .mtx in which a third of the entries come two or three times with different values -> parsed, merged with MAXIMUM,
    vertex-permuted -> three schedules -> every operator result against the oracle on the matrix the file describes: a merged
    duplicate that carried another value than the run's maximum shows in every result."""
    choose_setup(monkeypatch, host_setup)
    n, r, seed = 300, 16, 9
    path = str(tmp_path / "graph.mtx")
    rows, cols, vals = T.write_symmetric_mtx_with_duplicates(path, n, 4)
    label = O.vertex_permutation(n, seed)
    prow, pcol = label[rows], label[cols]
    order = np.argsort(prow * n + pcol)
    case = dict(name="mtx", M=n, N=n, R=r, rows=prow[order], cols=pcol[order], vals=vals[order], A=O.dense_fill(n, r, 31), B=O.dense_fill(n, r, 32))

    def from_file(w):
        sp = H.SpmatLocal.load_tuples(w, True, -1, -1, path)
        assert sp.info()["dist_nnz"] == len(rows)
        sp.permute(seed)
        return sp

    for alg, p, c in (("25d_dense_replicate", 8, 2), ("15d_fusion2", 4, 1), ("15d_fusion1", 1, 1)):
        per_rank = H.run_spmd(p, lambda w: T.run_all_ops(w, alg, c, case, make_spmat=from_file))
        assert per_rank[0]["alg_info"]["backend"] == "hip-gfx950"
        T.check_against_oracle(T.assemble(per_rank, case), case, alg)


@pytest.mark.parametrize("skewed", [False, True])
@pytest.mark.parametrize("host_setup", [False, True])
def test_generated_and_relabelled_input_equals_the_oracle_generator_hip(host_setup, skewed, monkeypatch):
    """SpmatLocal::loadTuples + permuteVertices describe the same matrix as the oracle's generator + oracle.vertex_permutation: the
    uniform initiator against oracle.erdos_renyi_mn, and HNH_RMAT=0.57,0.19,0.19 against oracle.rmat (loadTuples draws 2^logM *
    nnz_per_row edges with seed 12345 and scrambles by default: the oracle's defaults)."""
    choose_setup(monkeypatch, host_setup)
    monkeypatch.delenv("HNH_ER_SEED", raising=False)
    monkeypatch.delenv("HNH_RMAT_SCRAMBLE", raising=False)
    logm, ef, r, seed = 8, 8, 8, 5
    m = 1 << logm
    if skewed:
        monkeypatch.setenv("HNH_RMAT", "0.57,0.19,0.19")
        rows, cols = O.rmat(logm, m * ef, seed=12345)
    else:
        monkeypatch.delenv("HNH_RMAT", raising=False)
        rows, cols = O.erdos_renyi_mn(m, m, m * ef, 12345)
    perm = O.vertex_permutation(m, seed)
    case = T.make_case("gen8", m, m, r, perm[rows], perm[cols])

    def f(w):
        sp = H.SpmatLocal.load_tuples(w, False, logm, ef)
        info = sp.info()
        sp.permute(seed)
        d = H.DistributedSparse(w, "15d_fusion2", sp, r, 1)
        backend = d.json_algorithm_info()["backend"]
        A, B, S = d.like_A_matrix(0.0), d.like_B_matrix(0.0), d.like_S_values(1.0)
        subA, subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
        B.upload(T.fill_local(subB, B.shape, case["B"]))
        d.spmmA(A, B, S)
        out = dict(subA=subA, spmmA=A.download(), info=info, backend=backend)
        for x in (A, B, S):
            x.free()
        d.free(); sp.free()
        return out

    per_rank = H.run_spmd(4, f)
    assert per_rank[0]["backend"] == "hip-gfx950"
    assert per_rank[0]["info"]["dist_nnz"] == len(rows) and sum(o["info"]["local_nnz"] for o in per_rank) == len(rows)
    got = T.assemble_dense(per_rank, "spmmA", "subA", m, r)
    assert T.rel(got, O.spmm_a(case["rows"], case["cols"], np.ones(len(rows)), case["B"], m)) <= T.TOL


@pytest.mark.parametrize("case_name", ["rect_r16", "ragged_r8"])
@pytest.mark.parametrize("alg", H.ALGORITHMS)
def test_device_setup_places_every_nonzero_where_the_host_setup_does(alg, case_name, monkeypatch):
    """The device set-up (hnh_tuples_* on the GPU) against HNH_HOST_SETUP=1 on four ranks, rank by rank: the same nonzeros of S and of
    S^T on every rank (each rank's list ordered by row N + col), and over the ranks every edge of the input exactly once."""
    case = T.case_inputs(case_name)
    m, n = case["M"], case["N"]
    p, c = next((p, c) for p, c in ((4, 1), (4, 2)) if T.valid_config(alg, p, c, case["R"]))

    def rank(world):
        sp = H.SpmatLocal.from_global(world, m, n, case["rows"], case["cols"], case["vals"])
        d = H.DistributedSparse(world, alg, sp, case["R"], c)
        backend = d.json_algorithm_info()["backend"]
        sr, sc = d.S_coordinates()
        tr, tc = d.ST_coordinates()   # (rows of S^T are columns of S)
        d.free(); sp.free()
        return backend, np.sort(sr * n + sc), np.sort(tc * n + tr)

    placed = {}
    for host_setup in (False, True):
        choose_setup(monkeypatch, host_setup)
        placed[host_setup] = H.run_spmd(p, rank)
        assert all(r[0] == "hip-gfx950" for r in placed[host_setup])
    want = np.sort(case["rows"] * n + case["cols"])
    assert len(np.unique(want)) == len(want) > 0
    for k in (1, 2):
        for dev, host in zip(placed[False], placed[True]):
            assert np.array_equal(dev[k], host[k]), (alg, case_name, "S" if k == 1 else "S^T")
        for host_setup in (False, True):
            assert np.array_equal(np.sort(np.concatenate([r[k] for r in placed[host_setup]])), want), "every edge exactly once"
