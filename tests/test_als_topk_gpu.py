"""Top-k recommendation and ranking metrics for implicit-feedback ALS on the GPU (api.ImplicitALS.recommend / ranking_metrics; include/
hnh_topk.h: hnh_topk_rows_f64, hnh_topk_merge_f64, hnh_take_rows_f64; tests/als_topk_ref.py is the definition).

The kernel alone on small-integer operands (every score exact, ties plentiful): ids and scores EQUAL the definition at a covering subset of
nq in {0, 1, 15, 16, 17, 33, 70} x n in {0, 1, 9, 10, 63, 64, 65, 1000, 5000} x (R, k) in {(2, 1), (8, 10), (17, 2), (100, 64), (128, 128),
(130, 10), (256, 100), (320, 10), (512, 10)} (no query, one, either side of a 16-row fragment and of a wave's 32 rows, several waves; no
item, fewer than k, exactly k, k + 1, either side of a 64-item tile, many tiles; both kernel instances, remainders in R, with and without
16-byte loads), without lists and with random ones; with an empty list, a list that covers a whole item tile, one that leaves k - 1 items
and one that excludes everything.  Guard zones around every buffer are intact and the inputs unchanged.  splits in {1, 2, 3, 7} and the
library's choice, a query's position in a larger batch, and a second run all give the same bits.  Real operands pass check_topk at T.TOL.
The merge and the gather on exact operands; the refusals by message.  (The helpers are in tests/als_topk_common.py; more splits, hostile
item orders, odd bases and the larger merges: tests/test_als_topk_edges_gpu.py.)
The operator on loopback ranks: every rank the same arrays, check_topk against numpy on the factors, p > 1 bit-identical to p = 1, no seen
item with filter_seen, no padding id ever; ranking_metrics after two training steps on nine tenths of hub equals the definition."""
import ctypes as C
import functools

import numpy as np
import pytest

import als_common
import als_implicit_common as IC
import als_implicit_ref as IR
import als_topk_ref as TR
import hnh_testlib as T
from als_topk_common import Guarded, integers, random_lists, topk_rows
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu

NQS = (0, 1, 15, 16, 17, 33, 70)
NS = (0, 1, 9, 10, 63, 64, 65, 1000, 5000)
WIDTHS = ((2, 1), (8, 10), (17, 2), (100, 64), (128, 128), (130, 10), (256, 100), (320, 10), (512, 10))
# (nq, n, R, k): every value of each axis at least once; n < k, n == k and n == k + 1 at k = 64 and at k = 10
KERNEL_CASES = [(0, 64, 2, 1), (1, 0, 8, 10), (15, 1, 17, 2), (16, 9, 8, 10), (17, 10, 8, 10), (33, 63, 100, 64), (70, 64, 100, 64),
                (17, 65, 100, 64), (16, 1000, 128, 128), (70, 5000, 130, 10), (33, 1000, 256, 100), (15, 5000, 320, 10), (17, 1000, 512, 10),
                (70, 5000, 8, 10), (1, 5000, 2, 1), (33, 65, 128, 128)]
OPERATOR_CASES = [(8, 1, 1), (128, 1, 1), (128, 4, 1), (100, 5, 1), (100, 4, 2), (256, 4, 1)]


# ------------------------------------------------------------------------------------------------ the kernel, exact
@pytest.mark.parametrize("case", KERNEL_CASES, ids=als_common.case_id)
def test_topk_rows_is_exact_on_integers(ctx, case):
    nq, n, R, k = case
    rng = np.random.default_rng(hash(case) % 2**32)
    Q, Y = integers(rng, (nq, R)), integers(rng, (n, R))
    for excluded in (None, random_lists(rng, nq, n)):
        want_ids, want_scores = TR.topk(Q, Y, k, 10**10, excluded)
        ids, scores = topk_rows(ctx, Q, Y, k, 10**10, excluded)
        assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores)


def test_the_cases_are_the_ones_listed():
    assert len(KERNEL_CASES) == len(set(KERNEL_CASES)) == 16
    assert {c[0] for c in KERNEL_CASES} == set(NQS) and {c[1] for c in KERNEL_CASES} == set(NS) and {c[2:] for c in KERNEL_CASES} == set(WIDTHS)
    rel = {np.sign(n - k) if n != k + 1 else 2 for _, n, _, k in KERNEL_CASES}
    assert {-1, 0, 2} <= rel, "n < k, n == k and n == k + 1"
    assert len(OPERATOR_CASES) == len(set(OPERATOR_CASES)) == 6
    for R, p, c in OPERATOR_CASES:
        assert T.valid_config(IC.ALG, p, c, R)


@pytest.mark.parametrize("R,k", [(8, 10), (130, 10), (256, 100)])
def test_exclusion_never_shows_through(ctx, R, k):
    nq, n = 33, 1000
    rng = np.random.default_rng(R)
    Q, Y = integers(rng, (nq, R)), integers(rng, (n, R))
    S = Q @ Y.T
    excluded = random_lists(rng, nq, n)
    excluded[0] = np.arange(64, 128)                                      # a whole item tile
    excluded[1] = np.sort(rng.choice(n, size=n - (k - 1), replace=False))  # k - 1 items are left
    excluded[2] = np.arange(n)                                            # nothing is left
    excluded[3] = np.zeros(0, np.int64)                                   # an empty list among others
    excluded[4] = np.argsort(-S[4], kind="stable")[:200]                  # the 200 best items of the query
    excluded[4].sort()
    want_ids, want_scores = TR.topk(Q, Y, k, 5, excluded)
    for splits in (0, 1, 3):
        ids, scores = topk_rows(ctx, Q, Y, k, 5, excluded, splits)
        assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores)
    assert np.all(want_ids[2] == -1) and np.all(want_scores[2] == -np.inf) and np.sum(want_ids[1] >= 0) == k - 1
    # empty lists everywhere are no lists
    none = topk_rows(ctx, Q, Y, k, 5, None)
    empty = topk_rows(ctx, Q, Y, k, 5, [np.zeros(0, np.int64)] * nq)
    assert none[0].tobytes() == empty[0].tobytes() and none[1].tobytes() == empty[1].tobytes()


# ------------------------------------------------------------------------------------------------ the kernel, bits
@pytest.mark.parametrize("n", [65, 5000])
@pytest.mark.parametrize("R", [8, 130, 256])
def test_bits_do_not_depend_on_splits_position_or_run(ctx, n, R):
    rng = np.random.default_rng(n + R)
    k = 10
    Y = rng.standard_normal((n, R))
    mine = rng.standard_normal((5, R))
    excluded = random_lists(rng, 5, n)
    first = topk_rows(ctx, mine, Y, k, 0, excluded, 1)
    for splits in (1, 2, 3, 7, 0):  # (1 again: two runs are bit-equal)
        got = topk_rows(ctx, mine, Y, k, 0, excluded, splits)
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), splits
    # the same queries at other positions of a larger batch
    batch = rng.standard_normal((70, R))
    where = np.array([0, 15, 16, 33, 69])
    batch[where] = mine
    lists = random_lists(rng, 70, n)
    for q, e in zip(where, excluded):
        lists[q] = e
    got = topk_rows(ctx, batch, Y, k, 0, lists, 2)
    assert got[0][where].tobytes() == first[0].tobytes() and got[1][where].tobytes() == first[1].tobytes()
    # ... and items found through another base and another range keep their scores' bits
    shifted = topk_rows(ctx, mine, np.concatenate([rng.standard_normal((37, R)), Y]), n + 37, 0, None, 3) if n == 65 else None
    if shifted is not None:
        plain = topk_rows(ctx, mine, Y, n, 0, None, 1)
        for q in range(5):
            lookup = dict(zip(shifted[0][q].tolist(), shifted[1][q].tolist()))
            assert all(lookup[i + 37] == s for i, s in zip(plain[0][q].tolist(), plain[1][q].tolist()))


@pytest.mark.parametrize("R", [8, 128, 256])
def test_real_operands_pass_check_topk(ctx, R):
    c = IR.inputs("hub", R)
    Q, Y = np.ascontiguousarray(c["A"][:70]), np.ascontiguousarray(c["B"])
    rng = np.random.default_rng(R)
    excluded = random_lists(rng, 70, Y.shape[0])
    for k in (10, 128):
        ids, scores = topk_rows(ctx, Q, Y, k, 0, excluded)
        TR.check_topk(Q @ Y.T, excluded, ids, scores, k, T.TOL)


# ------------------------------------------------------------------------------------------------ merge, gather, refusals
@pytest.mark.parametrize("parts", [1, 2, 5, 8])
@pytest.mark.parametrize("n,k", [(100, 16), (1000, 10), (300, 128)])
def test_merge_reproduces_the_whole(ctx, parts, n, k):
    lib = K.load()
    nq, R = 17, 8
    rng = np.random.default_rng(parts * n)
    Q, Y = integers(rng, (nq, R)), integers(rng, (n, R))
    cuts = np.linspace(0, n, parts + 1).astype(int)
    lists = [TR.topk(Q, Y[a:b], k, 1000 + a) for a, b in zip(cuts[:-1], cuts[1:])]
    in_i, in_s = np.stack([x[0] for x in lists]), np.stack([x[1] for x in lists])
    if n < parts * k:
        assert np.any(in_i == -1), "parts with empty tails"
    in_s[in_i == -1] = 123.0  # the score of an empty entry is ignored
    want_ids, want_scores = TR.topk(Q, Y, k, 1000)
    bufs = [Guarded(ctx, a) for a in (in_s, in_i, np.full((nq, k), 7.5), np.full((nq, k), -7, np.int64))]
    ctx.check(lib.hnh_topk_merge_f64(ctx.h, bufs[0].ptr, bufs[1].ptr, parts, nq, k, bufs[2].ptr, bufs[3].ptr, K.STREAM_COMPUTE), "hnh_topk_merge_f64")
    got = [b.get() for b in bufs]
    for b in bufs:
        b.free()
    assert np.array_equal(got[0], in_s) and np.array_equal(got[1], in_i)
    assert np.array_equal(got[3], want_ids) and np.array_equal(got[2], want_scores)


@pytest.mark.parametrize("R", [1, 17, 128])
def test_take_rows(ctx, R):
    lib = K.load()
    rows = 50
    rng = np.random.default_rng(R)
    X = rng.standard_normal((rows, R))
    idx = np.array([3, -1, 49, 50, 0, 3, 10**12, -(10**12), 25], dtype=np.int64)
    bufs = [Guarded(ctx, a) for a in (X, idx, np.full((len(idx), R), 7.5))]
    ctx.check(lib.hnh_take_rows_f64(ctx.h, bufs[0].ptr, rows, R, bufs[1].ptr, len(idx), bufs[2].ptr, K.STREAM_COMPUTE), "hnh_take_rows_f64")
    got = [b.get() for b in bufs]
    for b in bufs:
        b.free()
    assert np.array_equal(got[0], X) and np.array_equal(got[1], idx)
    for q, src in enumerate(idx.tolist()):
        want = X[src] if 0 <= src < rows else np.zeros(R)
        assert got[2][q].tobytes() == want.tobytes(), (q, src)


def test_topk_refusals(ctx):
    lib = K.load()
    a = ctx.upload(np.zeros((4, 513)))
    y = ctx.upload(np.zeros((8, 513)))
    out = ctx.upload(np.zeros((4, 128)))
    work = ctx.upload(np.zeros(1 << 20, np.uint8))
    for nq, R, k, out_ptr, wb, text in ((4, 8, 0, out.ptr, 1 << 20, b"k must be between 1 and HNH_TOPK_MAX_K = 128"),
                                        (4, 8, 129, out.ptr, 1 << 20, b"k must be between 1 and HNH_TOPK_MAX_K = 128"),
                                        (4, 513, 10, out.ptr, 1 << 20, b"R must be between 1 and HNH_TOPK_MAX_R = 512"),
                                        (-1, 8, 10, out.ptr, 1 << 20, b"negative nq or n"),
                                        (4, 8, 10, None, 1 << 20, b"null pointer"),
                                        (4, 8, 10, out.ptr, 64, b"the workspace is too small")):
        rc = lib.hnh_topk_rows_f64(ctx.h, a.ptr, nq, y.ptr, 8, R, 0, None, None, k, 0, out_ptr, out.ptr, work.ptr, wb, K.STREAM_COMPUTE)
        assert rc != 0 and text in lib.hnh_last_error(ctx.h), lib.hnh_last_error(ctx.h)
    assert lib.hnh_topk_rows_f64_workspace(4, 8, 8, 0) == -1 and lib.hnh_topk_rows_f64_workspace(4, 8, 513, 10) == -1
    for x in (a, y, out, work):
        x.free()


# ------------------------------------------------------------------------------------------------ the operator
def users_of(case):
    m = case["M"]
    return np.array([1, m // 2, 7, m - 1, 1, 0, 500, m // 2 + 1], dtype=np.int64)  # two hub rows, the empty row, the last user, a repeat


def recommend_rank(world, c, case, users):
    s = IC.Solver(world, c, case, True)
    s.set(case["A"], case["B"])
    out = {(k, f): s.als.recommend(users, k, f) for k in (10, 128) for f in (True, False)}
    s.free()
    return out


@functools.lru_cache(maxsize=None)
def on_one_rank(R):
    case = IR.inputs("hub", R)
    return H.run_spmd(1, lambda w: recommend_rank(w, 1, case, users_of(case)))[0]


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=als_common.case_id)
def test_recommend_meets_numpy_on_every_rank_count(case):
    R, p, c = case
    inp = IR.inputs("hub", R)
    users = users_of(inp)
    per_rank = H.run_spmd(p, lambda w: recommend_rank(w, c, inp, users))
    S = inp["A"][users] @ inp["B"].T
    seen = [np.sort(inp["cols"][inp["rows"] == u]) for u in users]
    assert len(seen[0]) >= 1500 and len(seen[1]) >= 1100 and len(seen[2]) == 0
    for (k, filtered), (ids, scores) in per_rank[0].items():
        for other in per_rank[1:]:
            assert other[(k, filtered)][0].tobytes() == ids.tobytes() and other[(k, filtered)][1].tobytes() == scores.tobytes(), "every rank the same arrays"
        TR.check_topk(S, seen if filtered else None, ids, scores, k, T.TOL)
        assert ids.max() < inp["N"], "padding rows are never candidates"
        assert ids[0].tobytes() == ids[4].tobytes() and scores[0].tobytes() == scores[4].tobytes(), "a repeated user gets the same list"
        if filtered:
            for q, u in enumerate(users):
                assert not np.isin(ids[q], seen[q]).any()
        one = on_one_rank(R)[(k, filtered)]
        assert one[0].tobytes() == ids.tobytes() and one[1].tobytes() == scores.tobytes(), "bit-identical to one rank"
    # without the filter the hub users' lists hold seen items, and the empty column 11 appears wherever its score earns it
    ids, scores = per_rank[0][(128, False)]
    slack = T.TOL * np.max(np.abs(S))
    for q in range(len(users)):
        if q in (0, 1):
            assert np.isin(ids[q], seen[q]).any()
        if S[q, 11] > scores[q, -1] + slack:
            assert 11 in ids[q]


@pytest.mark.parametrize("p", [1, 4])
def test_ranking_metrics_after_training_equal_the_definition(p):
    R, k = 8, 10
    base = IR.inputs("hub", R)
    held = np.arange(len(base["rows"])) % 10 == 3
    train = dict(base, rows=base["rows"][~held], cols=base["cols"][~held], w=base["w"][~held], vals=base["vals"][~held])
    test_rows, test_cols = base["rows"][held], base["cols"][held]
    users = np.unique(test_rows)
    liked = [test_cols[test_rows == u] for u in users]

    def rank(world):
        s = IC.Solver(world, 1, train, True)
        s.set(train["A"], train["B"])
        s.als.run(2, 2)
        got = s.als.ranking_metrics(test_rows, test_cols, k=k, batch=1024)
        small = s.als.ranking_metrics(test_rows[::-1], test_cols[::-1], k=k, batch=97)
        ids, scores = s.als.recommend(users, k, True)
        a, b = s.get()
        out = dict(got=got, small=small, ids=ids, scores=scores, A=a, B=b, subA=s.subA, subB=s.subB)
        s.free()
        return out

    per_rank = H.run_spmd(p, rank)
    A = T.assemble_dense(per_rank, "A", "subA", base["M"], R)
    B = T.assemble_dense(per_rank, "B", "subB", base["N"], R)
    seen = [np.sort(train["cols"][train["rows"] == u]) for u in users]
    for o in per_rank:
        want = TR.ranking_metrics(o["ids"], liked, k)
        print("ranking metrics at p = %d: %s" % (p, o["got"]))
        assert o["got"]["users"] == want["users"] == len(users)
        for name in ("precision", "map", "ndcg"):
            assert abs(o["got"][name] - want[name]) <= 1e-15 and abs(o["small"][name] - want[name]) <= 1e-15, name
        assert o["ids"].tobytes() == per_rank[0]["ids"].tobytes()
        TR.check_topk(A[users] @ B.T, seen, o["ids"], o["scores"], k, T.TOL)
    assert 0.0 < per_rank[0]["got"]["precision"] <= 1.0, "held-out pairs are found: seen and held-out pairs are disjoint"
