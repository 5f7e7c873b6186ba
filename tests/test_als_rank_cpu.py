"""Exact item ranks and the rank metrics of implicit-feedback ALS without a GPU (api.ImplicitALS.rank_of / rank_metrics,
csrc/host/als_implicit.hpp, include/hnh_rank.h; tests/als_rank_ref.py is the definition).

The optional kernel group: declared == bound == exported by the HIP library, absent from both CPU test doubles, disjoint from every other
header and table, named in backend.hpp; the host call declared, bound and exported.
The host layer: rank_of and rank_metrics on either test double are refused with the missing-kernel message naming hnh_rank_rows_f64 and
its header (there is no host fallback), and the argument refusals come first, by name.
The definition: rank_counts() against a brute-force loop over the total order on small integers with plenty of ties; the AUC of
metrics() against brute-force counting of (positive, negative) pairs; MPR, AUC and MRR by hand on a five-user example (several held-out
items, a held-out item that is also seen, neg == 0, all scores tied, one candidate).
The condition of the GPU file's real-factor test: with its seed, the numpy model alone gives at least 99 % of the tested pairs an
allowance of 0."""
import ctypes as C
import os

import numpy as np
import pytest

import als_implicit_ref as IR
import als_rank_ref as RR
import hnh_testlib as T
from als_rank_common import REAL_CASES, real_pairs
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared

GROUP = {"hnh_pair_scores_f64", "hnh_rank_rows_f64_workspace", "hnh_rank_rows_f64", "hnh_rank_exclude_f64"}


# ------------------------------------------------------------------------------------------------ the group and the host call
def test_rank_is_an_optional_group():
    names = declared("hnh_rank.h")
    assert names == GROUP == set(K.RANK_SIGNATURES)
    for header in [h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h") and h != "hnh_rank.h"]:
        assert not names & declared(header), header
    for table in [n for n in dir(K) if n.endswith("SIGNATURES") and n != "RANK_SIGNATURES"]:
        assert not names & set(getattr(K, table)), table
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.RANK_SIGNATURES[n][1] and getattr(lib, n).restype == K.RANK_SIGNATURES[n][0]
    for path in (T.ORACLE_BACKEND, T.ORACLE_GAT_BACKEND):
        dbl = C.CDLL(path)
        for n in names:
            assert not hasattr(dbl, n), "the CPU test double %s does not export %s" % (os.path.basename(path), n)
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    text = open(os.path.join(ROOT, "include", "hnh_rank.h")).read()
    assert (K.RANK_MAX_R, K.RANK_MAX_TARGETS, K.RANK_MAX_SPLITS) == (512, 16, 1024)
    for line in ("#define HNH_RANK_MAX_R 512", "#define HNH_RANK_MAX_TARGETS 16", "#define HNH_RANK_MAX_SPLITS 1024"):
        assert line in text
    assert "NaN is NOT defined" in text, "the header says that behaviour on NaN is not defined"
    assert "No atomics on global memory" in text
    backend = open(os.path.join(ROOT, "distributed_sddmm_amd", "csrc", "host", "backend.hpp")).read()
    for n in names:
        assert 'X("include/hnh_rank.h", %s)' % n in backend
    # the workspace and the refusals of shapes need no device
    assert lib.hnh_rank_rows_f64_workspace(4, 100, 17 * 4, 0) == -1 and lib.hnh_rank_rows_f64_workspace(-1, 100, 0, 0) == -1
    assert lib.hnh_rank_rows_f64_workspace(4, 100, 8, 1025) == -1
    assert lib.hnh_rank_rows_f64_workspace(4, 100, 8, 1) == 48 and lib.hnh_rank_rows_f64_workspace(4, 100, 8, 3) == 48 + 3 * 8 * 8


def test_host_call_declared_and_exported():
    assert "hnh_ials_rank_of" in declared("hnh_dist.h") and "hnh_ials_rank_of" in H.SIGNATURES and hasattr(H.lib(), "hnh_ials_rank_of")
    assert callable(H.ImplicitALS.rank_of) and callable(H.ImplicitALS.rank_metrics)


# ------------------------------------------------------------------------------------------------ on the test doubles
@pytest.fixture(params=["plain", "gat"])
def double(request):
    path = T.ORACLE_BACKEND if request.param == "plain" else T.ORACLE_GAT_BACKEND
    H.load_backend(path)
    yield os.path.basename(path)
    H.load_backend(T.ORACLE_BACKEND)  # the modules after this one find the plain double, as before


def test_rank_of_is_refused_without_the_group_and_arguments_first(double):
    case = IR.inputs("rmat", 8)

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], case["vals"])
        d = H.DistributedSparse(world, "15d_fusion2", sp, 8, 1)
        als = H.ImplicitALS(d, 0.1)
        with pytest.raises(H.HnhError, match="Implicit_ALS rank_of needs initializeEmbeddings or set_embeddings first"):
            als.rank_of([0, 1], [2, 3])
        als.initializeEmbeddings()
        with pytest.raises(ValueError, match="as many users as items"):
            als.rank_of([0, 1], [2])
        for user in (-1, case["M"], case["M"] + 5):
            with pytest.raises(H.HnhError, match=r"Implicit_ALS rank_of: user %d is outside \[0, M = %d\)" % (user, case["M"])):
                als.rank_of([0, user, 1], [1, 1, 1])
        for item in (-1, case["N"], case["N"] + 5):
            with pytest.raises(H.HnhError, match=r"Implicit_ALS rank_of: item %d is outside \[0, N = %d\)" % (item, case["N"])):
                als.rank_of([0, 1, 1], [1, item, 1])
        missing = r"Implicit_ALS rank_of needs the kernel hnh_rank_rows_f64.*%s.*include/hnh_rank\.h" % double.replace(".", r"\.")
        for filter_seen in (True, False):
            with pytest.raises(H.HnhError, match=missing):
                als.rank_of([0, 1], [2, 3], filter_seen)
            with pytest.raises(H.HnhError, match=missing):
                als.rank_metrics(case["rows"][:5], case["cols"][:5], filter_seen=filter_seen)
        with pytest.raises(ValueError, match="batch >= 1"):
            als.rank_metrics(case["rows"][:5], case["cols"][:5], batch=0)
        als.free(); d.free()
        wide = H.DistributedSparse(world, "15d_fusion2", sp, 513, 1)
        als = H.ImplicitALS(wide, 0.1)
        als.initializeEmbeddings()
        with pytest.raises(H.HnhError, match=r"Implicit_ALS rank_of supports R <= HNH_RANK_MAX_R = 512, not R = 513"):
            als.rank_of([0, 1], [2, 3])
        als.free(); wide.free(); sp.free()
        return True

    assert H.run_spmd(1, rank) == [True]


# ------------------------------------------------------------------------------------------------ the definition
def brute_force_counts(scores, ids, ts, ti):
    count = 0
    for s, i in zip(scores, ids):
        if s > ts or (s == ts and i < ti):
            count += 1
    return count


@pytest.mark.parametrize("n,seed", [(0, 0), (1, 1), (40, 2), (65, 3)])
def test_rank_counts_is_the_total_order(n, seed):
    rng = np.random.default_rng(seed)
    scores = rng.integers(-2, 3, n).astype(np.float64)
    scores[rng.random(n) < 0.2] *= -0.0  # some zeros are -0.0: scores compare as numbers
    ids = 1000 + np.arange(n)
    tgt_score = np.concatenate([scores[:10], rng.integers(-3, 4, 10) + 0.5, rng.integers(-2, 3, 10), [0.0, -0.0]])
    tgt_id = np.concatenate([ids[:10], rng.integers(990, 1010 + n, 10), rng.integers(990, 1010 + n, 10), [1000 + n // 2] * 2])
    got = RR.rank_counts(scores, ids, tgt_score, tgt_id)
    want = [brute_force_counts(scores.tolist(), ids.tolist(), s, i) for s, i in zip(tgt_score.tolist(), tgt_id.tolist())]
    assert got.tolist() == want
    if n >= 40:
        assert len(np.unique(scores)) < n / 4, "the case has ties"
        assert got[-1] == got[-2], "-0.0 is +0.0"
        for t in range(10):  # an item's count is its index in the sorted order: it never ranks before itself
            assert got[t] == np.lexsort((ids, -scores)).tolist().index(t)
    # rows of queries, and the subtraction of excluded entries, are the same count
    Q, Y = rng.integers(-2, 3, (3, 4)).astype(np.float64), rng.integers(-2, 3, (n, 4)).astype(np.float64)
    ptr = np.array([0, 2, 2, 5])
    ts, ti = np.array([0.0, 1.5, -1.0, 2.0, 0.0]), np.array([1003, 7, 1001, 5000, 1000])
    rows = RR.rank_rows(Q, Y, 1000, ptr, ts, ti)
    S = Q @ Y.T if n else np.zeros((3, 0))
    assert rows.tolist() == [brute_force_counts(S[q].tolist(), ids.tolist(), ts[t], ti[t]) for q in range(3) for t in range(ptr[q], ptr[q + 1])]
    excl_ptr = np.array([0, n, n, n + min(n, 7)])
    es, ei = np.concatenate([S[0], S[2][:7]]), np.concatenate([ids, ids[:7]])
    left = RR.rank_exclude(rows, excl_ptr, es, ei, ptr, ts, ti)
    assert left[:2].tolist() == [0, 0] and left[2:].tolist() == [brute_force_counts(S[2][7:].tolist(), ids[7:].tolist(), ts[t], ti[t]) for t in (2, 3, 4)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_auc_is_the_share_of_rightly_ordered_pairs(seed):
    rng = np.random.default_rng(seed)
    m, n, R = 6, 30, 3
    A, B = rng.integers(-2, 3, (m, R)).astype(np.float64), rng.integers(-2, 3, (n, R)).astype(np.float64)
    rows, cols = rng.integers(0, m, 40), rng.integers(0, n, 40)
    seen = RR.seen_of(rows, cols)
    users, items = [], []
    for u in range(m):  # held-out items that the user has not seen, one to four a user
        free = np.setdiff1d(np.arange(n), seen.get(u, []))
        take = rng.choice(free, size=1 + u % 4, replace=False)
        users += [u] * len(take); items += take.tolist()
    for flt in (seen, None):
        ranks, cands = RR.rank_of(A, B, flt, users, items)
        got = RR.metrics(users, items, ranks, n, flt)
        want = []
        for u in range(m):
            held = [j for uu, j in zip(users, items) if uu == u]
            want.append(RR.auc_by_pairs(A[u] @ B.T, held, flt.get(u, []) if flt is not None else []))
        assert got["users"] == m and got["pairs"] == len(users)
        assert abs(got["auc"] - sum(want) / m) <= 1e-15
        assert np.all((0 <= ranks) & (ranks < cands))
        assert len(np.unique(A @ B.T)) < 40, "the case has ties"


def test_metrics_on_a_five_user_example():
    n = 6
    B = np.eye(n)
    A = np.array([[6.0, 5, 4, 3, 2, 1],   # user 0: strictly ordered, held out {1, 3}, has seen {0}
                  [1.0, 2, 3, 4, 5, 6],   # user 1: held out {5, 2}, has seen {5, 4}: the held-out item 5 is also seen
                  [1.0, 1, 2, 0, 0, 0],   # user 2: held out {0, 1}, has seen {2, 3, 4, 5}: no negative is left
                  [2.0, 2, 2, 2, 2, 2],   # user 3: all scores tied, held out {4}, has seen nothing
                  [0.0, 9, 1, 2, 3, 4]])  # user 4: held out {0}, has seen everything else: one candidate
    seen = {0: np.array([0]), 1: np.array([4, 5]), 2: np.array([2, 3, 4, 5]), 4: np.array([1, 2, 3, 4, 5])}
    users, items = [0, 0, 1, 1, 2, 2, 3, 4, 0], [1, 3, 5, 2, 0, 1, 4, 0, 3]  # (the pair (0, 3) twice)
    ranks, cands = RR.rank_of(A, B, seen, users, items)
    # user 0 without item 0: 1 is first, 3 has 1 and 2 before it.  user 1 without 4, 5: 5 is first of {0..3, 5}; 2 has 3 before it
    # (5 is excluded for 2).  user 2: candidates {0, 1}: 0 is first (the tie goes to the smaller id), 1 second.  user 3: four smaller ids.
    assert ranks.tolist() == [0, 2, 0, 1, 0, 1, 4, 0, 2] and cands.tolist() == [5, 5, 5, 4, 2, 2, 6, 1, 5]
    got = RR.metrics(users, items, ranks, n, seen)
    assert got["pairs"] == 8 and got["users"] == 3, "the repeated pair counts once; users 2 and 4 have neg == 0"
    mpr = (0 / 4 + 2 / 4 + 0 / 4 + 1 / 3 + 0 / 1 + 1 / 1 + 4 / 5 + 0) / 8
    # user 0: h = 2, neg = 6 - 1 - 2 = 3: 1 - (2 - 1) / 6.  user 1: h = 2, neg = 6 - |{4}| - 2 = 3: 1 - (1 - 1) / 6.  user 3: h = 1, neg = 5: 1 - 4 / 5
    auc = ((1 - 1 / 6) + 1.0 + (1 - 4 / 5)) / 3
    mrr = (1.0 + 1.0 + 1 / 5) / 3
    for name, value in (("mpr", mpr), ("auc", auc), ("mrr", mrr)):
        assert abs(got[name] - value) <= 1e-15, (name, got[name], value)
    # without the filter every item is a candidate
    ranks, cands = RR.rank_of(A, B, None, users, items)
    assert cands.tolist() == [6] * 9 and ranks.tolist() == [1, 3, 0, 3, 1, 2, 4, 5, 3]
    got = RR.metrics(users, items, ranks, n, None)
    assert got["users"] == 5 and abs(got["mrr"] - (1 / 2 + 1 + 1 / 2 + 1 / 5 + 1 / 6) / 5) <= 1e-15
    assert abs(got["mpr"] - (1 + 3 + 0 + 3 + 1 + 2 + 4 + 5) / 5 / 8) <= 1e-15
    assert abs(got["auc"] - ((1 - 3 / 8) + (1 - 2 / 8) + (1 - 2 / 8) + (1 - 4 / 5) + 0.0) / 5) <= 1e-15


# ------------------------------------------------------------------------------------------------ the condition of the real-factor test
@pytest.mark.parametrize("R", REAL_CASES)
def test_the_real_pairs_are_mostly_clear_of_ties(R):
    case = IR.inputs("hub", R)
    users, items = real_pairs(case)
    slack = T.TOL * np.max(np.abs(case["A"][np.unique(users)] @ case["B"].T))
    near = RR.near(case["A"], case["B"], users, items, slack)
    assert np.mean(near == 0) >= 0.99, "at least 99 %% of the pairs have no other score within the slack: %.4f" % np.mean(near == 0)
