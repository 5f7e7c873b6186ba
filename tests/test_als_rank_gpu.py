"""Exact item ranks and the rank metrics of implicit-feedback ALS on the GPU (api.ImplicitALS.rank_of / rank_metrics; include/hnh_rank.h:
hnh_pair_scores_f64, hnh_rank_rows_f64, hnh_rank_exclude_f64; tests/als_rank_ref.py is the definition, the guarded calls are in
tests/als_rank_common.py).

The kernels alone, exact.  On small-integer operands (every score exact in any order, ties plentiful) the counts EQUAL the definition at a
covering subset of nq in {0, 1, 15, 16, 17, 33, 70} x n in {0, 1, 63, 64, 65, 1000, 5000} x R in {2, 8, 17, 100, 128, 130, 256, 320, 512} x
targets per query in {0, 1, 2, 16} (either side of a fragment, a wave, an item tile, the boundary of the instance that keeps Q in
registers, and of the 16-byte-load condition), with targets that are real items, thresholds between scores, ties decided by the id and
repeats, ids from 10^10 on; guard zones intact, inputs unchanged; 17 targets in a row are refused and nothing is written.  All-tied
items ("flat", a zero Q, -0.0 mixed in): the count is the number of smaller ids.  Property 1: every score of hnh_topk_rows_f64's k = 128
lists equals hnh_pair_scores_f64's bit for bit, and hnh_rank_rows_f64 fed with them returns each item's index in the list.  Property 3:
splits, a second run, the query's position in a larger batch and partitions of Y give the same integers.  hnh_rank_exclude_f64 against
the definition.
The operator on loopback ranks: rank_of gives every item of recommend's lists its index, both ways of filter_seen, the same arrays on
every rank and for every rank count; integer factors EQUAL numpy; real factors differ from numpy's rank by at most the number of scores
within T.TOL max|S| of the target's; rank_metrics after two training steps equals the definition applied to rank_of's integers."""
import functools

import numpy as np
import pytest

import als_common
import als_implicit_common as IC
import als_implicit_ref as IR
import als_rank_ref as RR
import hnh_testlib as T
from als_rank_common import REAL_CASES, mixed_targets, pair_scores, rank_exclude, rank_rows, real_pairs, targets_per_row
from als_topk_common import integers, ordered_case, topk_rows
from distributed_sddmm_amd import api as H
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu

NQS = (0, 1, 15, 16, 17, 33, 70)
NS = (0, 1, 63, 64, 65, 1000, 5000)
RS = (2, 8, 17, 100, 128, 130, 256, 320, 512)
PER_ROW = (0, 1, 2, 16)
# (nq, n, R, the most targets of a row): every value of each axis at least once
KERNEL_CASES = [(0, 64, 2, 1), (1, 0, 8, 2), (15, 1, 17, 16), (16, 63, 8, 1), (17, 64, 100, 2), (33, 65, 128, 16), (70, 1000, 130, 1),
                (33, 5000, 256, 2), (15, 1000, 320, 16), (17, 5000, 512, 1), (70, 5000, 8, 16), (1, 5000, 2, 2), (16, 1000, 128, 0),
                (33, 64, 100, 1), (70, 65, 256, 16), (17, 1000, 17, 2)]
OPERATOR_CASES = [(8, 1, 1), (128, 4, 1), (100, 4, 2), (256, 4, 1)]
ID_BASE = 10**10


# ------------------------------------------------------------------------------------------------ the kernels, exact
@pytest.mark.parametrize("case", KERNEL_CASES, ids=als_common.case_id)
def test_counts_are_exact_on_integers(ctx, case):
    nq, n, R, most = case
    rng = np.random.default_rng(hash(case) % 2**32)
    Q, Y = integers(rng, (nq, R)), integers(rng, (n, R))
    S = Q @ Y.T if n else np.zeros((nq, 0))
    tgt_ptr = targets_per_row(rng, nq, most)
    tgt_score, tgt_id = mixed_targets(rng, S, ID_BASE, tgt_ptr)
    want = RR.rank_rows(Q, Y, ID_BASE, tgt_ptr, tgt_score, tgt_id)
    shift = 8 if case[0] == 70 else 0  # bases that forbid the 16-byte loads although R allows them
    got = rank_rows(ctx, Q, Y, ID_BASE, tgt_ptr, tgt_score, tgt_id, shift_q=shift, shift_y=shift)
    assert np.array_equal(got, want)
    if n > 1 and len(want):
        assert want.max() > 0 and len(np.unique(S)) < S.size


def test_the_cases_are_the_ones_listed():
    assert len(KERNEL_CASES) == len(set(KERNEL_CASES)) == 16
    assert {c[0] for c in KERNEL_CASES} == set(NQS) and {c[1] for c in KERNEL_CASES} == set(NS)
    assert {c[2] for c in KERNEL_CASES} == set(RS) and {c[3] for c in KERNEL_CASES} == set(PER_ROW)
    assert set(OPERATOR_CASES) == {(8, 1, 1), (128, 4, 1), (100, 4, 2), (256, 4, 1)}
    for R, p, c in OPERATOR_CASES:
        assert T.valid_config(IC.ALG, p, c, R)
    assert set(REAL_CASES) == {c[0] for c in OPERATOR_CASES}


def test_seventeen_targets_in_a_row_are_refused(ctx):
    rng = np.random.default_rng(17)
    Q, Y = integers(rng, (3, 8)), integers(rng, (100, 8))
    for ptr in ([0, 16, 33, 34], [0, 17, 17, 17]):
        rank_rows(ctx, Q, Y, 0, np.array(ptr), np.zeros(ptr[-1]), np.arange(ptr[-1]), refused="more than HNH_RANK_MAX_TARGETS = 16")
    rank_rows(ctx, Q, Y, 0, np.array([0, 2, 1, 3]), np.zeros(3), np.arange(3), refused="tgt_ptr must ascend")
    rank_rows(ctx, Q, Y, -1, np.array([0, 1, 2, 3]), np.zeros(3), np.arange(3), refused="id_base must be between 0 and INT64_MAX - n")
    rank_rows(ctx, Q, Y, 0, np.array([0, 1, 2, 3]), np.zeros(3), np.arange(3), splits=1025, refused="splits must be between 0 and HNH_RANK_MAX_SPLITS")
    assert np.array_equal(rank_rows(ctx, Q, Y, 0, np.array([0, 16, 16, 32]), np.full(32, 1000.0), np.arange(32)), np.zeros(32, np.int64))


@pytest.mark.parametrize("R", [8, 130])
def test_ties_are_decided_by_the_id(ctx, R):
    nq, n = 17, 1000
    rng = np.random.default_rng(R)
    tgt_ptr = targets_per_row(rng, nq, 16)
    items = rng.integers(0, n, int(tgt_ptr[nq]))
    rows = np.repeat(np.arange(nq), np.diff(tgt_ptr))
    Q, Y = ordered_case("flat", nq, n, R)
    flat = rank_rows(ctx, Q, Y, ID_BASE, tgt_ptr, (Q @ Y.T)[rows, items], ID_BASE + items)
    assert np.array_equal(flat, items), "the count of a target is the number of smaller ids"
    # a zero Q: every score is a zero; -0.0 mixed into both operands and the targets: scores compare as numbers
    Qz = np.where(rng.random((nq, R)) < 0.5, -0.0, 0.0)
    Yn = Y * np.where(rng.random((n, R)) < 0.5, -1.0, 1.0)
    signed = np.where(rng.random(len(items)) < 0.5, -0.0, 0.0)
    assert np.signbit(Qz).any() and np.signbit(signed).any() and not np.signbit(signed).all()
    assert np.array_equal(rank_rows(ctx, Qz, Yn, ID_BASE, tgt_ptr, signed, ID_BASE + items), items)


# ------------------------------------------------------------------------------------------------ property 1: the very bits
@pytest.mark.parametrize("R", [8, 17, 128, 130, 256, 512])
def test_pair_scores_are_the_bits_of_topk_and_ranks_its_indices(ctx, R):
    nq, n, k = 33, 200, 128
    rng = np.random.default_rng(R)
    Q, Y = rng.standard_normal((nq, R)), rng.standard_normal((n, R))
    ids, scores = topk_rows(ctx, Q, Y, k)
    assert ids.min() >= 0
    pair_q = np.repeat(np.arange(nq), k)
    got = pair_scores(ctx, Q, Y, pair_q, ids.reshape(-1))
    assert np.array_equal(got.view(np.int64), scores.reshape(-1).view(np.int64)), "bit for bit"
    assert np.max(np.abs(got - np.einsum("ij,ij->i", Q[pair_q], Y[ids.reshape(-1)]))) <= T.TOL * np.max(np.abs(scores))
    # a query with 128 targets becomes eight query rows of 16
    rows = np.repeat(np.arange(nq), k // 16)
    tgt_ptr = 16 * np.arange(len(rows) + 1)
    counts = rank_rows(ctx, np.ascontiguousarray(Q[rows]), Y, 0, tgt_ptr, got, ids.reshape(-1))
    assert np.array_equal(counts.reshape(nq, k), np.tile(np.arange(k), (nq, 1))), "every item's index in the list"
    # pairs out of range, either way, give +0.0
    bad_q = np.array([0, 1, -1, nq, 2, 10**12], dtype=np.int64)
    bad_j = np.array([-1, n, 3, 4, 10**12, -5], dtype=np.int64)
    zeros = pair_scores(ctx, Q, Y, bad_q, bad_j, shift_q=8)
    assert np.all(zeros.view(np.int64) == 0)
    assert len(pair_scores(ctx, Q, Y, [], [])) == 0 and np.all(pair_scores(ctx, Q, Y[:0], [0, 1], [0, 1]).view(np.int64) == 0)


# ------------------------------------------------------------------------------------------------ property 3: additivity
@pytest.mark.parametrize("n", [65, 5000])
@pytest.mark.parametrize("R", [8, 130, 256])
def test_counts_do_not_depend_on_splits_position_run_or_partition(ctx, n, R):
    rng = np.random.default_rng(n + R)
    Y = rng.standard_normal((n, R))
    mine = rng.standard_normal((5, R))
    tgt_ptr = np.array([0, 16, 17, 17, 25, 41])
    rows = np.repeat(np.arange(5), np.diff(tgt_ptr))
    items = rng.integers(0, n, len(rows))
    tgt_score = pair_scores(ctx, mine, Y, rows, items)
    tgt_score[::5] += 1e-3  # some thresholds that are no item's score
    tgt_id = 1000 + items
    first = rank_rows(ctx, mine, Y, 1000, tgt_ptr, tgt_score, tgt_id, 1)
    near = RR.rank_rows(mine, Y, 1000, tgt_ptr, tgt_score, tgt_id)
    assert np.max(np.abs(first - near)) <= 2 and first.max() > n // 2, "numpy's scores may swap neighbours"
    for splits in (1, 2, 3, 7, 0):  # (1 again: two runs give the same integers)
        assert np.array_equal(rank_rows(ctx, mine, Y, 1000, tgt_ptr, tgt_score, tgt_id, splits), first), splits
    # the same queries at other positions of a larger batch, among rows with targets of their own
    batch = rng.standard_normal((70, R))
    where = np.array([0, 15, 16, 33, 69])
    batch[where] = mine
    per = rng.integers(0, 17, 70)
    per[where] = np.diff(tgt_ptr)
    big_ptr = np.concatenate([[0], np.cumsum(per)])
    big_score, big_id = rng.standard_normal(big_ptr[-1]), rng.integers(0, 2000 + n, big_ptr[-1])
    for q, (a, b) in zip(where, zip(tgt_ptr[:-1], tgt_ptr[1:])):
        big_score[big_ptr[q]:big_ptr[q + 1]], big_id[big_ptr[q]:big_ptr[q + 1]] = tgt_score[a:b], tgt_id[a:b]
    got = rank_rows(ctx, batch, Y, 1000, big_ptr, big_score, big_id, 2)
    assert np.array_equal(np.concatenate([got[big_ptr[q]:big_ptr[q + 1]] for q in where]), first)
    # Y in parts, each with its id_base: the counts add up
    for parts in (1, 2, 5):
        cuts = np.linspace(0, n, parts + 1).astype(int)
        total = sum(rank_rows(ctx, mine, np.ascontiguousarray(Y[a:b]), 1000 + a, tgt_ptr, tgt_score, tgt_id) for a, b in zip(cuts[:-1], cuts[1:]))
        assert np.array_equal(total, first), parts


# ------------------------------------------------------------------------------------------------ the subtraction
def test_exclude_subtracts_what_ranks_before(ctx):
    rng = np.random.default_rng(5)
    nq, n = 6, 300
    tgt_ptr = np.array([0, 3, 3, 20, 21, 30, 46])
    tgt_score = rng.integers(-3, 4, tgt_ptr[-1]).astype(np.float64)
    tgt_id = rng.integers(0, n, tgt_ptr[-1])
    lists = [np.zeros(0, np.int64), np.arange(5), np.arange(n), np.array([tgt_id[20]]), np.sort(rng.choice(n, 70, replace=False)), np.arange(0, n, 2)]
    excl_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    excl_id = np.concatenate(lists)
    excl_score = rng.integers(-3, 4, len(excl_id)).astype(np.float64)
    excl_score[excl_ptr[3]] = tgt_score[20]  # the list of query 3 holds the target itself: it does not rank before itself
    counts = rng.integers(0, 10**12, tgt_ptr[-1])
    want = RR.rank_exclude(counts, excl_ptr, excl_score, excl_id, tgt_ptr, tgt_score, tgt_id)
    got = rank_exclude(ctx, counts, excl_ptr, excl_score, excl_id, tgt_ptr, tgt_score, tgt_id)
    assert np.array_equal(got, want)
    assert got[20] == counts[20] and np.array_equal(got[:3], counts[:3]) and np.any(got[3:20] != counts[3:20])


# ------------------------------------------------------------------------------------------------ the operator
def users_of(case):
    m = case["M"]
    return np.array([1, m // 2, 7, m - 1, 1, 0, 500, m // 2 + 1], dtype=np.int64)  # two hub rows, the empty row, the last user, a repeat


def operator_rank(world, c, case, users, integer):
    s = IC.Solver(world, c, case, True)
    A, B = (np.rint(4 * case["A"]), np.rint(4 * case["B"])) if integer else (case["A"], case["B"])
    s.set(A, B)
    out = {}
    if integer:
        pu, pi = real_pairs(case)
        out["int"] = {f: s.als.rank_of(pu, pi, f) for f in (True, False)}
    else:
        for f in (True, False):
            ids, _ = s.als.recommend(users, 128, f)
            out[("list", f)] = ids
            out[("rank", f)] = s.als.rank_of(np.repeat(users, 128), ids.reshape(-1), f)
        seen_pairs = [(u, j) for u in users[:2] for j in case["cols"][case["rows"] == u][:40]]
        out["seen"] = s.als.rank_of([u for u, _ in seen_pairs], [j for _, j in seen_pairs], True)
        out["seen_pairs"] = np.array(seen_pairs)
        pu, pi = real_pairs(case)
        out["real"] = {f: s.als.rank_of(pu, pi, f) for f in (True, False)}
    s.free()
    return out


@functools.lru_cache(maxsize=None)
def on_one_rank(R, integer):
    case = IR.inputs("hub", R)
    return H.run_spmd(1, lambda w: operator_rank(w, 1, case, users_of(case), integer))[0]


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=als_common.case_id)
def test_rank_of_is_the_index_in_recommend(case):
    R, p, c = case
    inp = IR.inputs("hub", R)
    users = users_of(inp)
    per_rank = H.run_spmd(p, lambda w: operator_rank(w, c, inp, users, False))
    for other in per_rank[1:]:
        assert same(other, per_rank[0]), "every rank the same arrays"
    assert same(per_rank[0], on_one_rank(R, False)), "the same integers as one rank"
    out = per_rank[0]
    seen = RR.seen_of(inp["rows"], inp["cols"])
    for f in (True, False):
        ranks, cands = out[("rank", f)]
        assert ranks.dtype == np.int64 and cands.dtype == np.int64 and out[("list", f)].min() >= 0
        assert np.array_equal(ranks.reshape(len(users), 128), np.tile(np.arange(128), (len(users), 1))), "the item's index in recommend's list"
        want = [inp["N"] - (len(seen.get(int(u), [])) if f else 0) for u in users]  # (a recommended item is never a seen one under the filter)
        assert np.array_equal(cands.reshape(len(users), 128), np.repeat(np.array(want)[:, None], 128, axis=1))
    # seen items of the hub users under the filter: ranked among the unseen ones, the item itself counted in
    ranks, cands = out["seen"]
    pairs = out["seen_pairs"]
    assert len(pairs) == 80 and np.all((0 <= ranks) & (ranks < cands))
    assert np.array_equal(cands, np.array([inp["N"] - (len(seen[int(u)]) - 1) for u, _ in pairs]))
    # real factors against numpy: the rank may differ by the number of scores within the slack of the target's
    pu, pi = real_pairs(inp)
    slack = T.TOL * np.max(np.abs(inp["A"][np.unique(pu)] @ inp["B"].T))
    near = RR.near(inp["A"], inp["B"], pu, pi, slack)
    assert np.mean(near == 0) >= 0.99
    for f in (True, False):
        want_ranks, want_cands = RR.rank_of(inp["A"], inp["B"], seen if f else None, pu, pi)
        ranks, cands = out["real"][f]
        assert np.array_equal(cands, want_cands), "candidates equal the definition"
        assert np.all(np.abs(ranks - want_ranks) <= near), np.max(np.abs(ranks - want_ranks) - near)


@pytest.mark.parametrize("case", OPERATOR_CASES, ids=als_common.case_id)
def test_rank_of_equals_numpy_on_integer_factors(case):
    R, p, c = case
    inp = IR.inputs("hub", R)
    per_rank = H.run_spmd(p, lambda w: operator_rank(w, c, inp, users_of(inp), True))
    for other in per_rank[1:]:
        assert same(other, per_rank[0])
    assert same(per_rank[0], on_one_rank(R, True))
    A, B = np.rint(4 * inp["A"]), np.rint(4 * inp["B"])
    assert np.abs(A).max() <= 64 and len(np.unique(A[:50] @ B.T)) < 50 * inp["N"] / 4, "small integers: every score is exact, ties are plentiful"
    pu, pi = real_pairs(inp)
    seen = RR.seen_of(inp["rows"], inp["cols"])
    for f in (True, False):
        want_ranks, want_cands = RR.rank_of(A, B, seen if f else None, pu, pi)
        ranks, cands = per_rank[0]["int"][f]
        assert np.array_equal(ranks, want_ranks) and np.array_equal(cands, want_cands)


@pytest.mark.parametrize("p", [1, 4])
def test_rank_metrics_after_training_equal_the_definition(p):
    R = 8
    base = IR.inputs("hub", R)
    held = np.arange(len(base["rows"])) % 10 == 3
    train = dict(base, rows=base["rows"][~held], cols=base["cols"][~held], w=base["w"][~held], vals=base["vals"][~held])
    test_rows, test_cols = base["rows"][held], base["cols"][held]

    def rank(world):
        s = IC.Solver(world, 1, train, True)
        s.set(train["A"], train["B"])
        s.als.run(2, 2)
        out = dict(got={f: s.als.rank_metrics(test_rows, test_cols, batch=1024, filter_seen=f) for f in (True, False)},
                   small=s.als.rank_metrics(np.concatenate([test_rows[::-1], test_rows[:50]]), np.concatenate([test_cols[::-1], test_cols[:50]]), batch=97),
                   ranks={f: s.als.rank_of(test_rows, test_cols, f) for f in (True, False)})
        s.free()
        return out

    per_rank = H.run_spmd(p, rank)
    seen = RR.seen_of(train["rows"], train["cols"])
    for o in per_rank:
        for f in (True, False):
            ranks, cands = o["ranks"][f]
            assert np.array_equal(ranks, per_rank[0]["ranks"][f][0]) and np.all((0 <= ranks) & (ranks < cands))
            want = RR.metrics(test_rows, test_cols, ranks, base["N"], seen if f else None)
            got = o["got"][f]
            print("rank metrics at p = %d, filter_seen = %s: %s" % (p, f, got))
            assert got["users"] == want["users"] and got["pairs"] == want["pairs"] == len(np.unique(test_rows * base["N"] + test_cols))
            for name in ("mpr", "auc", "mrr"):
                assert abs(got[name] - want[name]) <= 1e-15, (name, got[name], want[name])
            if f:
                assert got["mpr"] < 0.5 < got["auc"]
        for name in ("mpr", "auc", "mrr", "users", "pairs"):
            assert abs(o["small"][name] - o["got"][True][name]) <= 1e-15, "batch = 97, reversed and repeated pairs give the same numbers"
