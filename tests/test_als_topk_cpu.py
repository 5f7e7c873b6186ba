"""Top-k recommendation and ranking metrics for implicit-feedback ALS without a GPU (api.ImplicitALS.recommend / ranking_metrics,
csrc/host/als_implicit.hpp, include/hnh_topk.h; tests/als_topk_ref.py is the definition).

The builders of hostile item orders (als_topk_common.ordered_case, used by tests/test_als_topk_edges_gpu.py): exact scores, the answers
they are meant to have, one item per tile for "trickle", and an emulation of a lazily raised threshold (als_topk_common.lazy_cuts) that
says at which (have, add) the candidate buffer is cut at the shapes the GPU tests use.
The definition: topk() against a brute-force loop over the total order (with plenty of ties) and against torch.topk where no two scores
are equal; the three metrics against values computed by hand on a six-user example (a user with more held-out items than k, a user whose
list has -1 entries, a user with no hit).
The optional kernel group: declared == bound == exported by the HIP library, absent from both CPU test doubles.
The host layer: recommend on either test double is refused with the missing-kernel message naming hnh_topk_rows_f64 and its header (there
is no host fallback), and the argument refusals come first, by name."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import als_implicit_ref as IR
import als_topk_common as TC
import als_topk_ref as TR
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared

GROUP = {"hnh_topk_rows_f64_workspace", "hnh_topk_rows_f64", "hnh_topk_merge_f64", "hnh_take_rows_f64"}


# ------------------------------------------------------------------------------------------------ the definition
def brute_force(Q, Y, k, id_base, excluded):
    ids, scores = [], []
    for q in range(Q.shape[0]):
        cand = [(float(Q[q] @ Y[j]), id_base + j) for j in range(Y.shape[0]) if j not in set(excluded[q])]
        best = []
        while cand and len(best) < k:  # repeatedly the first candidate of the total order
            top = cand[0]
            for c in cand[1:]:
                if c[0] > top[0] or (c[0] == top[0] and c[1] < top[1]):
                    top = c
            cand.remove(top)
            best.append(top)
        best += [(-np.inf, -1)] * (k - len(best))
        scores.append([b[0] for b in best]); ids.append([b[1] for b in best])
    return np.array(ids, dtype=np.int64).reshape(Q.shape[0], k), np.array(scores).reshape(Q.shape[0], k)


@pytest.mark.parametrize("nq,n,R,k", [(3, 40, 4, 5), (2, 7, 3, 7), (2, 6, 3, 7), (1, 0, 2, 3), (4, 65, 2, 10)])
def test_topk_is_the_total_order(nq, n, R, k):
    rng = np.random.default_rng(100 * n + k)
    Q, Y = rng.integers(-2, 3, (nq, R)).astype(np.float64), rng.integers(-2, 3, (n, R)).astype(np.float64)
    excluded = [np.sort(rng.choice(n, size=min(n, q), replace=False)) for q in range(nq)]
    ids, scores = TR.topk(Q, Y, k, 1000, excluded)
    want_ids, want_scores = brute_force(Q, Y, k, 1000, excluded)
    assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores)
    if n:
        assert len(np.unique(Q @ Y.T)) < nq * n, "the case has ties"
    TR.check_topk(Q @ Y.T if n else np.zeros((nq, 0)), excluded, ids, scores, k, 0.0, id_base=1000)


def test_topk_is_torch_topk_without_ties():
    rng = np.random.default_rng(3)
    Q, Y = rng.standard_normal((5, 16)), rng.standard_normal((300, 16))
    S = Q @ Y.T
    assert len(np.unique(S)) == S.size
    ids, scores = TR.topk(Q, Y, 20)
    want = torch.topk(torch.from_numpy(S), 20, dim=1)
    assert np.array_equal(ids, want.indices.numpy()) and np.array_equal(scores, want.values.numpy())
    TR.check_topk(S, None, ids, scores, 20, T.TOL)


def test_check_topk_catches_what_it_should():
    rng = np.random.default_rng(4)
    Q, Y = rng.standard_normal((2, 8)), rng.standard_normal((50, 8))
    S, excluded = Q @ Y.T, [np.array([3, 4]), np.array([], dtype=np.int64)]
    ids, scores = TR.topk(Q, Y, 5, 0, excluded)
    TR.check_topk(S, excluded, ids, scores, 5, T.TOL)
    for spoil in ("excluded", "repeat", "order", "missed", "score"):
        i, s = ids.copy(), scores.copy()
        if spoil == "excluded":
            i[0, 4], s[0, 4] = 3, S[0, 3]
        elif spoil == "repeat":
            i[1, 1], s[1, 1] = i[1, 0], s[1, 0]
        elif spoil == "order":
            i[1, [0, 1]], s[1, [0, 1]] = i[1, [1, 0]], s[1, [1, 0]]
        elif spoil == "missed":
            worst = int(np.argmin(S[1]))
            i[1, 4], s[1, 4] = worst, S[1, worst]
        else:
            s[0, 2] += 1e-6
        with pytest.raises(AssertionError):
            TR.check_topk(S, excluded, i, s, 5, T.TOL)


def test_metrics_on_a_six_user_example():
    k = 3
    ids = np.array([[5, 2, 9], [1, 7, 3], [4, -1, -1], [1, 2, 3], [8, 6, 0], [-1, -1, -1]])
    liked = [[5, 9], [1, 2, 3, 4, 5], [4], [9], [0], [2, 3]]  # user 1: |L| > k; user 2: -1 entries; users 3 and 5: no hit
    a = 1.0 / np.log2(3.0)
    want = dict(precision=6 / 10,                                         # hits 2 + 2 + 1 + 0 + 1 + 0 over m = 2 + 3 + 1 + 1 + 1 + 2
                map=(5 / 6 + 5 / 9 + 1 + 0 + 1 / 3 + 0) / 6,              # (1 + 2/3) / 2, (1 + 2/3) / 3, 1, 0, (1/3) / 1, 0
                ndcg=(1.5 / (1 + a) + 1.5 / (1.5 + a) + 1 + 0 + 0.5 + 0) / 6)  # hits at ranks 1 and 3: 1 + 1/2; ideal: 1 + a (+ 1/2)
    got = TR.ranking_metrics(ids, liked, k)
    assert got["users"] == 6
    for name, value in want.items():
        assert abs(got[name] - value) <= 1e-15, (name, got[name], value)


# ------------------------------------------------------------------------------------------------ the hostile item orders
ORDERED_N = 16640  # the items of the GPU tests' long cases: 260 tiles


@pytest.mark.parametrize("kind", TC.KINDS)
def test_ordered_scores_are_exact_and_ordered_alike(kind):
    nq, n, R = 5, 2000, 132
    Q, Y = TC.ordered_case(kind, nq, n, R)
    v = TC.ordered_values(kind, n)
    assert Q.shape == (nq, R) and Y.shape == (n, R) and Q.flags.c_contiguous and Y.flags.c_contiguous
    assert np.all((Q >= 1) & (Q <= 3) & (Q == np.rint(Q))) and np.array_equal(Y, np.outer(v, np.ones(R)))
    S = Q @ Y.T
    assert np.array_equal(S, np.outer(Q.sum(axis=1), v)) and np.array_equal(S, np.rint(S)), "every score is v_j * sum(Q[q]), an integer"
    # ... and so is every partial sum, in any order of the products: |Q| <= 3 and the largest tested |v| bound them far below 2^53
    assert 3 * 512 * (ORDERED_N + 1) < 2**53 and np.max(np.abs(TC.ordered_values(kind, ORDERED_N))) <= ORDERED_N
    Q2, Y2 = TC.ordered_case(kind, nq, n, R)
    assert Q2.tobytes() == Q.tobytes() and Y2.tobytes() == Y.tobytes(), "the builder is a function of its arguments"


@pytest.mark.parametrize("k", [10, 64, 65, 128])
def test_ordered_cases_have_the_answers_they_are_meant_to(k):
    nq, n, R = 3, 2000, 4
    rng = np.random.default_rng(k)
    excluded = TC.random_lists(rng, nq, n)
    excluded[0] = np.arange(n - 5, n)  # the five best of "ascending"
    excluded[1] = np.arange(0, 7)      # the seven first of "flat"
    for lists in (None, excluded):
        left = [np.setdiff1d(np.arange(n), lists[q] if lists is not None else []) for q in range(nq)]
        Q, Y = TC.ordered_case("ascending", nq, n, R)
        ids, scores = TR.topk(Q, Y, k, 0, lists)
        for q in range(nq):
            assert np.array_equal(ids[q], left[q][::-1][:k]), "the last k ids that are left, descending"
            assert np.array_equal(scores[q], ids[q] * Q[q].sum())
        Q, Y = TC.ordered_case("flat", nq, n, R)
        ids, scores = TR.topk(Q, Y, k, 0, lists)
        for q in range(nq):
            assert np.array_equal(ids[q], left[q][:k]) and np.all(scores[q] == 5 * Q[q].sum()), "the first k ids that are left"
        Q, Y = TC.ordered_case("descending", nq, n, R)
        ids, _ = TR.topk(Q, Y, k, 0, lists)
        for q in range(nq):
            assert np.array_equal(ids[q], left[q][:k])


@pytest.mark.parametrize("k", [10, 64, 65, 100])
def test_trickle_brings_one_item_per_tile(k):
    n = ORDERED_N
    v = TC.ordered_values("trickle", n)
    tiles = n // TC.ITEM_TILE
    spikes = np.array([TC.ITEM_TILE * t + (7 * t) % TC.ITEM_TILE for t in range(tiles)])
    assert n % TC.ITEM_TILE == 0 and tiles == 260 and np.array_equal(v[spikes], np.arange(tiles) + 1) and np.all(np.delete(v, spikes) < 0)
    assert len({int(s) % TC.ITEM_TILE for s in spikes[:64]}) == 64, "the spike visits every lane"
    best = np.zeros(0, dtype=np.int64)  # the ids of the running first k, kept exactly: a sequential pass over the tiles
    for t in range(tiles):
        js = np.arange(TC.ITEM_TILE * t, TC.ITEM_TILE * (t + 1))
        if t >= -(-k // TC.ITEM_TILE):  # from tile 1 on for k <= 64, from tile 2 on for k <= 128: before that there is no k-th best yet
            kth = best[-1]  # (v has no ties: "ranks before" is v > v[kth])
            assert len(best) == k and np.sum(v[js] > v[kth]) == 1 and v[spikes[t]] > v[kth], t
        else:
            assert len(best) < k
        both = np.concatenate([best, js])
        best = both[np.lexsort((both, -v[both]))][:k]
    assert np.array_equal(best, spikes[::-1][:k]), "the top-k is the last k spikes"
    Q, Y = TC.ordered_case("trickle", 2, n, 3)
    ids, scores = TR.topk(Q, Y, k)
    assert np.array_equal(ids, np.stack([spikes[::-1][:k]] * 2)) and np.array_equal(scores[1], v[ids[1]] * Q[1].sum())


def test_the_orders_reach_the_cuts():
    """If someone shrinks n or moves k, this says that the kernel's cut paths are no longer reached by the GPU tests' inputs."""
    cap = lambda k: 128 if k <= 64 else 256  # noqa: E731  (topk_cap of hnh_topk_kernels.hpp)
    trickle, ascending = TC.ordered_values("trickle", ORDERED_N), TC.ordered_values("ascending", ORDERED_N)
    for k in (10, 64):
        assert (128, 1) in TC.lazy_cuts(trickle, k, cap(k)), k
    for k in (65, 100):
        assert (256, 1) in TC.lazy_cuts(trickle, k, cap(k)), k
    assert (128, 64) in TC.lazy_cuts(ascending, 64, cap(64)) and (128, 64) in TC.lazy_cuts(ascending, 10, cap(10))
    assert (256, 64) in TC.lazy_cuts(ascending, 128, cap(128))
    assert (193, 64) in TC.lazy_cuts(ascending, 65, cap(65)), "k + 2 tiles fit, the third does not"
    # ascending cuts whenever the buffer is full, a last tile of 16 items included; descending and flat cut once: nothing passes the
    # first threshold ...
    assert TC.lazy_cuts(ascending[:2000], 64, 128) == {(128, 64), (128, 16)}
    for kind in ("descending", "flat"):
        assert TC.lazy_cuts(TC.ordered_values(kind, ORDERED_N), 10, 128) == {(128, 64)}, kind
        assert TC.lazy_cuts(TC.ordered_values(kind, ORDERED_N), 100, 256) == {(256, 64)}, kind
    # ... and the emulation itself on five tiles that can be followed by hand (k = 2, cap = 128; equal values: the smaller index first)
    v = np.full(320, -1000)
    v[[0, 1, 2]] = [5, 6, 7]  # tiles 0 and 1 fill the buffer; tile 2 cuts it at (128, 64) to {7, 6}, threshold (6, 1), and brings 64
    v[192:255] = 100          # tile 3: 63 pass, 66 + 63 > 128: cut at (66, 63), the threshold stays (6, 1), have = 65
    v[[260, 261]] = [6, 9]    # tile 4: 6 ties with the threshold at a larger index and fails, 9 passes, 66 fit
    assert TC.lazy_cuts(v, 2, 128) == {(128, 64), (66, 63)}
    assert TC.lazy_cuts(v[:192], 2, 128) == {(128, 64)} and TC.lazy_cuts(v[:128], 2, 128) == set()


# ------------------------------------------------------------------------------------------------ the group and the host call
def test_topk_is_an_optional_group():
    names = declared("hnh_topk.h")
    assert names == GROUP == set(K.TOPK_SIGNATURES)
    for header in [h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h") and h != "hnh_topk.h"]:
        assert not names & declared(header), header
    for table in [n for n in dir(K) if n.endswith("SIGNATURES") and n != "TOPK_SIGNATURES"]:
        assert not names & set(getattr(K, table)), table
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.TOPK_SIGNATURES[n][1] and getattr(lib, n).restype == K.TOPK_SIGNATURES[n][0]
    for path in (T.ORACLE_BACKEND, T.ORACLE_GAT_BACKEND):
        dbl = C.CDLL(path)
        for n in names:
            assert not hasattr(dbl, n), "the CPU test double %s does not export %s" % (os.path.basename(path), n)
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    text = open(os.path.join(ROOT, "include", "hnh_topk.h")).read()
    assert (K.TOPK_MAX_K, K.TOPK_MAX_R, K.TOPK_MAX_SPLITS) == (128, 512, 1024)
    for line in ("#define HNH_TOPK_MAX_K 128", "#define HNH_TOPK_MAX_R 512", "#define HNH_TOPK_MAX_SPLITS 1024"):
        assert line in text
    assert "NaN is NOT defined" in text, "the header says that behaviour on NaN is not defined"
    backend = open(os.path.join(ROOT, "distributed_sddmm_amd", "csrc", "host", "backend.hpp")).read()
    for n in names:
        assert 'X("include/hnh_topk.h", %s)' % n in backend


def test_host_call_declared_and_exported():
    assert "hnh_ials_recommend" in declared("hnh_dist.h") and "hnh_ials_recommend" in H.SIGNATURES and hasattr(H.lib(), "hnh_ials_recommend")
    assert callable(H.ImplicitALS.recommend) and callable(H.ImplicitALS.ranking_metrics)


# ------------------------------------------------------------------------------------------------ on the test doubles
@pytest.fixture(params=["plain", "gat"])
def double(request):
    path = T.ORACLE_BACKEND if request.param == "plain" else T.ORACLE_GAT_BACKEND
    H.load_backend(path)
    yield os.path.basename(path)
    H.load_backend(T.ORACLE_BACKEND)  # the modules after this one find the plain double, as before


def test_recommend_is_refused_without_the_group_and_arguments_first(double):
    case = IR.inputs("rmat", 8)

    def rank(world):
        sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], case["vals"])
        d = H.DistributedSparse(world, "15d_fusion2", sp, 8, 1)
        als = H.ImplicitALS(d, 0.1)
        with pytest.raises(H.HnhError, match="Implicit_ALS recommend needs initializeEmbeddings or set_embeddings first"):
            als.recommend([0, 1], 3)
        als.initializeEmbeddings()
        for k in (0, -1, 129):
            with pytest.raises(H.HnhError, match=r"Implicit_ALS recommend needs 1 <= k <= HNH_TOPK_MAX_K = 128, not k = %d" % k):
                als.recommend([0, 1], k)
        for user in (-1, case["M"], case["M"] + 5):
            with pytest.raises(H.HnhError, match=r"Implicit_ALS recommend: user %d is outside \[0, M = %d\)" % (user, case["M"])):
                als.recommend([0, user, 1], 3)
        missing = r"Implicit_ALS recommend needs the kernel hnh_topk_rows_f64.*%s.*include/hnh_topk\.h" % double.replace(".", r"\.")
        for filter_seen in (True, False):
            with pytest.raises(H.HnhError, match=missing):
                als.recommend([0, 1], 3, filter_seen)
        with pytest.raises(H.HnhError, match=missing):
            als.ranking_metrics(case["rows"][:5], case["cols"][:5], k=3)
        als.free(); d.free()
        wide = H.DistributedSparse(world, "15d_fusion2", sp, 513, 1)
        als = H.ImplicitALS(wide, 0.1)
        als.initializeEmbeddings()
        with pytest.raises(H.HnhError, match=r"Implicit_ALS recommend supports R <= HNH_TOPK_MAX_R = 512, not R = 513"):
            als.recommend([0, 1], 3)
        als.free(); wide.free(); sp.free()
        return True

    assert H.run_spmd(1, rank) == [True]
