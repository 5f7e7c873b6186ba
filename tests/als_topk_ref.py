"""The numpy definition of top-k recommendation and of the ranking metrics (api.ImplicitALS.recommend / ranking_metrics,
include/hnh_topk.h).

The total order: candidate (s, id) ranks before (s', id') when s > s', or when s == s' and id < id'.  topk() is np.lexsort on
(id, -score); check_topk() is for real-valued operands, where two scores within rounding may legitimately swap; the metrics are those of
the `implicit` package's ranking_metrics_at_k."""
import numpy as np

NEG_INF = -np.inf


def topk(Q, Y, k, id_base=0, excluded=None):
    """(ids int64 [nq, k], scores [nq, k]): the first k items of every query row in the total order of (<Q_q, Y_j>, id_base + j), without
    the local rows excluded[q]; the tail is (-1, -inf)."""
    nq, n = Q.shape[0], Y.shape[0]
    S = Q @ Y.T if n else np.zeros((nq, 0))
    ids = np.full((nq, k), -1, dtype=np.int64)
    scores = np.full((nq, k), NEG_INF)
    for q in range(nq):
        keep = np.ones(n, dtype=bool)
        if excluded is not None and len(excluded[q]):
            keep[np.asarray(excluded[q], dtype=np.int64)] = False
        cand = np.nonzero(keep)[0]
        order = cand[np.lexsort((cand, -S[q, cand]))][:k]
        ids[q, :len(order)] = id_base + order
        scores[q, :len(order)] = S[q, order]
    return ids, scores


def check_topk(S, excluded, ids, scores, k, tol, id_base=0):
    """Every property of a correct answer for real-valued scores S [nq, n] (the reference's), to tol * max|S|."""
    nq, n = S.shape
    assert ids.shape == (nq, k) and scores.shape == (nq, k)
    slack = tol * (np.max(np.abs(S)) if S.size else 0.0)
    for q in range(nq):
        out = np.zeros(n, dtype=bool)
        if excluded is not None and len(excluded[q]):
            out[np.asarray(excluded[q], dtype=np.int64)] = True
        available = int(n - out.sum())
        filled = min(k, available)
        got, sc = ids[q, :filled] - id_base, scores[q, :filled]
        assert np.all(ids[q, filled:] == -1) and np.all(scores[q, filled:] == NEG_INF), "exactly max(0, k - available) trailing (-1, -inf)"
        assert np.all((got >= 0) & (got < n)), "ids in range"
        assert len(np.unique(got)) == filled, "ids distinct"
        assert not np.any(out[got]), "no excluded item"
        assert np.all(np.abs(sc - S[q, got]) <= slack), "every score is the item's"
        assert np.all(sc[:-1] >= sc[1:]), "scores non-increasing"
        ties = sc[:-1] == sc[1:]
        assert np.all(got[:-1][ties] < got[1:][ties]), "equal neighbours have ascending ids"
        rest = ~out
        rest[got] = False
        if filled and rest.any():
            assert sc.min() >= S[q, rest].max() - slack, "nothing better was left behind"


def ranking_metrics(ids, liked, k):
    """precision, map, ndcg at k and the number of users: ids [users, k] (entries -1 are misses), liked[u] the user's held-out items."""
    discount = 1.0 / np.log2(np.arange(2, k + 2))
    hits_total = m_total = ap = ndcg = 0.0
    for row, held in zip(ids, liked):
        held = set(int(x) for x in held)
        m = min(k, len(held))
        hits = 0
        ap_u = dcg = 0.0
        for t, item in enumerate(row[:k], start=1):
            if int(item) >= 0 and int(item) in held:
                hits += 1
                ap_u += hits / t
                dcg += discount[t - 1]
        hits_total += hits
        m_total += m
        ap += ap_u / m
        ndcg += dcg / discount[:m].sum()
    users = len(ids)
    return dict(precision=hits_total / m_total, map=ap / users, ndcg=ndcg / users, users=users)
