"""The numpy definition of exact item ranks and of the rank metrics (api.ImplicitALS.rank_of / rank_metrics, include/hnh_rank.h).

The total order is that of tests/als_topk_ref.py: candidate (s, id) ranks before (s', id') when s > s', or when s == s' and id < id'; an
item never ranks before itself.  rank_counts() counts the candidates that rank before a target; rank_of() is the operator's answer from
dense factors; metrics() turns integer ranks into MPR (the expected percentile rank of Hu, Koren and Volinsky with r_ui = 1), AUC and MRR.
Sums of floating-point terms are exactly rounded (math.fsum), so they do not depend on the order of the terms."""
import math

import numpy as np


def before(s, i, ts, ti):
    """(s, i) ranks before (ts, ti), elementwise"""
    return (s > ts) | ((s == ts) & (i < ti))


def rank_counts(scores, ids, tgt_score, tgt_id):
    """counts[t] = #{ j : (scores[j], ids[j]) ranks before (tgt_score[t], tgt_id[t]) } for the candidates of ONE query"""
    scores, ids = np.asarray(scores, dtype=np.float64), np.asarray(ids, dtype=np.int64)
    return np.array([int(np.sum(before(scores, ids, s, i))) for s, i in zip(np.asarray(tgt_score).tolist(), np.asarray(tgt_id).tolist())],
                    dtype=np.int64).reshape(-1)


def rank_rows(Q, Y, id_base, tgt_ptr, tgt_score, tgt_id):
    """hnh_rank_rows_f64: the counts of every query row's targets over the items of Y (ids id_base + j), numpy scores"""
    nq, n = Q.shape[0], Y.shape[0]
    S = Q @ Y.T if n else np.zeros((nq, 0))
    ids = id_base + np.arange(n, dtype=np.int64)
    out = np.zeros(int(tgt_ptr[nq]) if nq else 0, dtype=np.int64)
    for q in range(nq):
        a, b = int(tgt_ptr[q]), int(tgt_ptr[q + 1])
        out[a:b] = rank_counts(S[q], ids, tgt_score[a:b], tgt_id[a:b])
    return out


def rank_exclude(counts, excl_ptr, excl_score, excl_id, tgt_ptr, tgt_score, tgt_id):
    """hnh_rank_exclude_f64: counts minus the excluded entries of the target's query that rank before the target"""
    out = np.array(counts, dtype=np.int64)
    for q in range(len(tgt_ptr) - 1):
        e0, e1, a, b = int(excl_ptr[q]), int(excl_ptr[q + 1]), int(tgt_ptr[q]), int(tgt_ptr[q + 1])
        out[a:b] -= rank_counts(excl_score[e0:e1], excl_id[e0:e1], tgt_score[a:b], tgt_id[a:b])
    return out


def seen_of(rows, cols):
    """user -> the sorted distinct items of the user's row of S"""
    out = {}
    for u in np.unique(rows).tolist():
        out[u] = np.unique(cols[rows == u])
    return out


def rank_of(A, B, seen, users, items):
    """(ranks, candidates) of the pairs from dense factors: the candidates of user u are all N items without seen[u] (seen: a dict
    user -> items, or None: no filter) and always with the asked item; rank = the candidates other than the item that rank before it."""
    n = B.shape[0]
    ranks, cands = np.zeros(len(users), np.int64), np.zeros(len(users), np.int64)
    ids = np.arange(n, dtype=np.int64)
    for i, (u, item) in enumerate(zip(np.asarray(users).tolist(), np.asarray(items).tolist())):
        s = A[u] @ B.T
        keep = np.ones(n, dtype=bool)
        if seen is not None and u in seen:
            keep[seen[u]] = False
        keep[item] = False
        ranks[i] = int(np.sum(before(s[keep], ids[keep], s[item], item)))
        cands[i] = int(keep.sum()) + 1
    return ranks, cands


def near(A, B, users, items, slack):
    """near[i] = the number of items other than items[i] whose numpy score for users[i] lies within `slack` of the item's: as many places
    may a rank computed from scores with other rounding differ"""
    out = np.zeros(len(users), np.int64)
    for i, (u, item) in enumerate(zip(np.asarray(users).tolist(), np.asarray(items).tolist())):
        s = A[u] @ B.T
        out[i] = int(np.sum(np.abs(s - s[item]) <= slack)) - 1
    return out


def metrics(users, items, ranks, n_items, seen=None):
    """dict(mpr, auc, mrr, users, pairs) of held-out pairs with their integer ranks (duplicates of a pair are dropped); seen: a dict
    user -> items of S (the filter of rank_of), or None.  With L_u the held-out items of user u and h = |L_u|:
        candidates of a pair = n_items - |seen_u \\ {item}|
        mpr = mean over the pairs of rank / (candidates - 1), 0 where candidates == 1
        auc = mean over the users of 1 - (sum_t rank_t - h (h - 1) / 2) / (h neg),  neg = n_items - |seen_u \\ L_u| - h
        mrr = mean over the users of 1 / (1 + min_t rank_t)
    Users with neg == 0 are left out of auc and mrr and are not counted in `users`."""
    table = {}
    for u, j, r in zip(np.asarray(users).tolist(), np.asarray(items).tolist(), np.asarray(ranks).tolist()):
        assert table.setdefault((u, j), r) == r, "a repeated pair has one rank"
    per_user = {}
    pr = []
    for (u, j), r in sorted(table.items()):
        mine = set(seen[u].tolist()) if seen is not None and u in seen else set()
        cand = n_items - len(mine - {j})
        assert 0 <= r < cand
        pr.append(r / (cand - 1) if cand > 1 else 0.0)
        per_user.setdefault(u, []).append((j, r))
    auc, rr = [], []
    for u, held in sorted(per_user.items()):
        mine = set(seen[u].tolist()) if seen is not None and u in seen else set()
        h = len(held)
        neg = n_items - len(mine - {j for j, _ in held}) - h
        if neg == 0:
            continue
        auc.append(1.0 - (sum(r for _, r in held) - h * (h - 1) // 2) / (h * neg))
        rr.append(1.0 / (1 + min(r for _, r in held)))
    mean = lambda v: math.fsum(v) / len(v) if v else 0.0  # noqa: E731
    return dict(mpr=mean(pr), auc=mean(auc), mrr=mean(rr), users=len(auc), pairs=len(pr))


def auc_by_pairs(scores, positives, excluded):
    """The AUC of ONE user by brute force: the share of (positive, negative) pairs in which the positive ranks before the negative, the
    negatives being every item that is neither positive nor excluded; None where there is no negative"""
    n = len(scores)
    pos = set(int(j) for j in positives)
    out = set(int(j) for j in excluded)
    negs = [j for j in range(n) if j not in pos and j not in out]
    if not negs:
        return None
    right = sum(1 for p in pos for j in negs if scores[p] > scores[j] or (scores[p] == scores[j] and p < j))
    return right / (len(pos) * len(negs))
