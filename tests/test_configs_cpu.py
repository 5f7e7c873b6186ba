"""BASELINE.json configurations as parity-test cases on CPU ranks (host logic + transports; kernels served by
the oracle test double):  config 1 exactly (ER 2^16, ~1e6 nnz, R = 16, 1.5D sparse shift, world = 2 over gloo) and
the shape of config 4 (skewed graph, 2.5D dense-replicate, p = 8, c = 2) on an R-MAT stand-in."""
import numpy as np
import pytest

import hnh_testlib as T
from distributed_sddmm_amd import api as H
from oracle import oracle as O
from world_launch import launch


@pytest.fixture(autouse=True, scope="module")
def cpu_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    yield


def test_rmat_generator_twin_and_skew():
    r1, c1 = H.generate_rmat(12, 4096 * 16)
    r2, c2 = O.rmat(12, 4096 * 16)
    assert np.array_equal(r1, r2) and np.array_equal(c1, c2)
    deg = np.bincount(r1, minlength=4096)
    assert deg.max() > 20 * deg.mean(), "R-MAT must be skewed (hub rows)"


def test_config1_sparse_shift_world2_gloo():
    procs, outs = launch(2, "cfg1", "15d_sparse:1", timeout=600)
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    assert "GLOO_OK" in outs[0], outs[0][-2000:]


@pytest.mark.parametrize("alg,p,c", [("25d_dense_replicate", 8, 2), ("25d_sparse_replicate", 8, 2), ("15d_fusion2", 8, 2), ("15d_sparse", 4, 1)])
def test_config4_shape_skewed_graph(alg, p, c):
    rows, cols = H.generate_rmat(10, 1024 * 12)
    case = T.make_case("rmat10", 1024, 1024, 32, rows, cols)
    per_rank = H.run_spmd(p, lambda w: T.run_all_ops(w, alg, c, case))
    imbalance = per_rank[0]["alg_info"]["nnz_procs"]
    assert sum(imbalance) == len(rows) * (c if alg == "25d_sparse_replicate" else 1) or sum(imbalance) == len(rows)
    T.check_against_oracle(T.assemble(per_rank, case), case, alg)


def test_vertex_permutation_balances_a_skewed_graph_and_commutes_with_the_operator():
    """SpmatLocal::permuteVertices (the reference's random_permute.cpp / RenameVertices step): P S P^T.  The operator
    on the relabelled matrix with relabelled dense operands gives the relabelled result, and the per-rank nonzero
    counts of a skewed graph get closer to uniform."""
    rows, cols = H.generate_rmat(10, 1024 * 12, scramble=False)  # hubs clustered at small vertex ids
    m, r, seed = 1024, 16, 77
    case = T.make_case("rmat10", m, m, r, rows, cols)
    perm = O.vertex_permutation(m, seed)

    def body(permute):
        def f(w):
            sp = H.SpmatLocal.from_global(w, m, m, rows, cols, case["vals"])
            if permute:
                sp.permute(seed)
            d = H.DistributedSparse(w, "15d_fusion2", sp, r, 1)
            A, B, S = d.like_A_matrix(0.0), d.like_B_matrix(0.0), d.like_S_values(1.0)
            subA, subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
            bg = case["B"]
            if permute:
                bg = np.empty_like(case["B"]); bg[perm] = case["B"]
            B.upload(T.fill_local(subB, B.shape, bg))
            d.spmmA(A, B, S)
            out = dict(subA=subA, spmmA=A.download(), nnz=d.json_algorithm_info()["nnz_procs"])
            d.free(); sp.free()
            return out
        return f

    plain = H.run_spmd(4, body(False))
    shuf = H.run_spmd(4, body(True))
    a0 = T.assemble_dense(plain, "spmmA", "subA", m, r)
    a1 = T.assemble_dense(shuf, "spmmA", "subA", m, r)
    assert T.rel(a1[perm], a0) <= T.TOL  # (P S P^T)(P B) = P (S B)
    imb = lambda c: max(c) / (sum(c) / len(c))  # noqa: E731
    assert imb(shuf[0]["nnz"]) < imb(plain[0]["nnz"])


@pytest.mark.parametrize("host_setup", [False, True])
def test_generated_and_relabelled_input_equals_the_oracle_generator(host_setup, monkeypatch):
    """SpmatLocal::loadTuples + permuteVertices (device-resident by default, host with HNH_HOST_SETUP=1) describe the same
    matrix as oracle.erdos_renyi_mn + oracle.vertex_permutation: same nonzero count, same operator result."""
    if host_setup:
        monkeypatch.setenv("HNH_HOST_SETUP", "1")
    logm, ef, r, seed = 8, 8, 8, 5
    m = 1 << logm
    rows, cols = O.erdos_renyi_mn(m, m, m * ef, 12345)
    perm = O.vertex_permutation(m, seed)
    case = T.make_case("gen8", m, m, r, perm[rows], perm[cols])

    def f(w):
        sp = H.SpmatLocal.load_tuples(w, False, logm, ef)
        info = sp.info()
        sp.permute(seed)
        d = H.DistributedSparse(w, "15d_fusion2", sp, r, 1)
        A, B, S = d.like_A_matrix(0.0), d.like_B_matrix(0.0), d.like_S_values(1.0)
        subA, subB = d.submatrices(H.AMAT), d.submatrices(H.BMAT)
        B.upload(T.fill_local(subB, B.shape, case["B"]))
        d.spmmA(A, B, S)
        out = dict(subA=subA, spmmA=A.download(), info=info)
        d.free(); sp.free()
        return out

    per_rank = H.run_spmd(4, f)
    assert per_rank[0]["info"]["dist_nnz"] == len(rows) and sum(o["info"]["local_nnz"] for o in per_rank) == len(rows)
    got = T.assemble_dense(per_rank, "spmmA", "subA", m, r)
    assert T.rel(got, O.spmm_a(case["rows"], case["cols"], np.ones(len(rows)), case["B"], m)) <= T.TOL


def test_config1_full_size_against_the_compiled_reference():
    """BASELINE config 1 at its full size (ER 2^16, edge factor 16, ~1.05e6 nonzeros, R = 16, 1.5D sparse shift, world = 2):
    the scratch.cpp fingerprints (squared norms of SDDMM / SpMM-A / SpMM-B results under the dummyInitialize fill) of
    the REFERENCE ITSELF (oracle/_ref/ref_driver under mpiexec -n 2) against ours on two CPU ranks.  Only where the compiled
    reference exists (this container); the committed golden vectors cover the small cases everywhere."""
    from oracle import refrun as RR
    if not RR.available():
        pytest.skip("compiled reference not available on this box")
    m, r = 1 << 16, 16
    rows, cols = O.erdos_renyi_mn(m, m, m * 16, 12345)
    ref = RR.fingerprints(m, m, rows, cols, r, "15d_sparse", 2, 1, timeout=600)
    case = T.make_case("cfg1", m, m, r, rows, cols)
    per_rank = H.run_spmd(2, lambda w: T.run_all_ops(w, "15d_sparse", 1, case))
    ours = np.sum([o["fingerprints"] for o in per_rank], axis=0)
    want = np.array([ref["sddmm"], ref["spmmA"], ref["spmmB"]]) if isinstance(ref, dict) else np.asarray(ref)
    assert T.rel(ours, want) <= T.TOL, (ours, want)


@pytest.mark.parametrize("host_setup", [False, True])
def test_matrix_market_file_through_the_schedules(tmp_path, monkeypatch, host_setup):
    """SURVEY 8(f3) on the CPU test double: symmetric .mtx with duplicates -> parsed, merged with maximum (device-style
    pipeline: sort + hnh_tuples_dedup_max, or the host pipeline), vertex-permuted -> 2.5D dense-replicate and 1.5D fused ->
    every operator result against the oracle on the matrix the file describes."""
    if host_setup:
        monkeypatch.setenv("HNH_HOST_SETUP", "1")
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

    for alg, p, c in (("25d_dense_replicate", 8, 2), ("15d_fusion2", 4, 1)):
        per_rank = H.run_spmd(p, lambda w: T.run_all_ops(w, alg, c, case, make_spmat=from_file))
        T.check_against_oracle(T.assemble(per_rank, case), case, alg)


@pytest.mark.parametrize("host_setup", [False, True])
def test_matrix_market_parser_survives_untidy_files(tmp_path, monkeypatch, host_setup):
    """The parser cuts the memory-mapped text into one piece per thread at line boundaries and reads indices with its own
    digit loop: a general (rectangular) real file with CRLF line ends, tabs, leading blanks, exponents, comment and blank lines
    inside the body and no line feed after the last entry must give exactly the matrix scipy reads from it."""
    import scipy.io
    if host_setup:
        monkeypatch.setenv("HNH_HOST_SETUP", "1")
    m, n, r = 70, 53, 8
    rng = np.random.default_rng(5)
    keys = rng.choice(m * n, 900, replace=False)
    vals = rng.uniform(-1, 1, len(keys)) * 10.0 ** rng.integers(-3, 4, len(keys))
    lines = []
    for k, v in zip(keys.tolist(), vals.tolist()):
        sep = rng.choice([" ", "\t", "   "])
        lead = rng.choice(["", " ", "\t"])
        num = ("%.17e" % v) if rng.random() < 0.5 else repr(v)
        lines.append("%s%d%s%d%s%s" % (lead, k // n + 1, sep, k % n + 1, sep, num))
        if rng.random() < 0.05:
            lines.append("% a comment in the body")
        if rng.random() < 0.05:
            lines.append("")
    text = "%%MatrixMarket matrix coordinate real general\r\n% header comment\r\n" + "%d %d %d\r\n" % (m, n, len(keys)) + "\r\n".join(lines)
    path = str(tmp_path / "untidy.mtx")
    with open(path, "w", newline="") as f:
        f.write(text)  # no line end after the last entry
    tidy = str(tmp_path / "tidy.mtx")
    with open(tidy, "w") as f:  # what scipy is given: the same entries, conventionally formatted
        f.write("%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (m, n, len(keys)))
        for k, v in zip(keys.tolist(), vals.tolist()):
            f.write("%d %d %r\n" % (k // n + 1, k % n + 1, v))
    ref = scipy.io.mmread(tidy).tocoo()
    order = np.argsort(ref.row.astype(np.int64) * n + ref.col)
    case = dict(name="untidy", M=m, N=n, R=r, rows=ref.row[order].astype(np.int64), cols=ref.col[order].astype(np.int64), vals=ref.data[order],
                A=O.dense_fill(m, r, 31), B=O.dense_fill(n, r, 32))

    def from_file(w):
        sp = H.SpmatLocal.load_tuples(w, True, -1, -1, path)
        assert sp.info()["dist_nnz"] == len(keys) and sp.info()["M"] == m and sp.info()["N"] == n
        return sp

    per_rank = H.run_spmd(4, lambda w: T.run_all_ops(w, "15d_fusion2", 1, case, make_spmat=from_file))
    T.check_against_oracle(T.assemble(per_rank, case), case, "15d_fusion2")
