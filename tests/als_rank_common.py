"""What the rank tests share (tests/test_als_rank_gpu.py, tests/test_als_rank_cpu.py; include/hnh_rank.h): the guarded calls of
hnh_pair_scores_f64, hnh_rank_rows_f64 and hnh_rank_exclude_f64 (every buffer between guard zones, als_topk_common.Pack / Scratch; the guard
zones are checked and the inputs compared after the call), and the builders of targets.  A plain module, no conftest: nothing here
touches a GPU until a function is called with a ctx."""
import ctypes as C

import numpy as np

from als_topk_common import Pack, Scratch
from distributed_sddmm_amd import _kernels as K

UNTOUCHED = -7  # what the outputs hold before a call
REAL_SEED = 11  # the seed of the pairs of the real-factor tests (here and in tests/test_als_rank_gpu.py)
REAL_CASES = (8, 128, 100, 256)


def real_pairs(case, seed=REAL_SEED, count=300):
    """The (user, item) pairs of the real-factor tests: random users and items of the case, the hub rows among them"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, case["M"], count)
    users[:40] = np.array([1, case["M"] // 2] * 20)
    return users.astype(np.int64), rng.integers(0, case["N"], count).astype(np.int64)


def pair_scores(ctx, Q, Y, pair_q, pair_j, shift_q=0, shift_y=0):
    """hnh_pair_scores_f64 between guard zones; returns the scores"""
    lib = K.load()
    (nq, R), n, npairs = Q.shape, Y.shape[0], len(pair_q)
    pair_q, pair_j = np.asarray(pair_q, dtype=np.int64), np.asarray(pair_j, dtype=np.int64)
    bufs = Pack(ctx, Q=(Q if nq else np.zeros((1, R)), shift_q), Y=(Y if n else np.zeros((1, R)), shift_y), q=(pair_q if npairs else np.zeros(1, np.int64), 0),
                j=(pair_j if npairs else np.zeros(1, np.int64), 0), out=(np.full(max(npairs, 1), 7.5), 0))
    ctx.check(lib.hnh_pair_scores_f64(ctx.h, bufs.ptr("Q"), nq, bufs.ptr("Y"), n, R, bufs.ptr("q"), bufs.ptr("j"), npairs, bufs.ptr("out"), K.STREAM_COMPUTE),
              "hnh_pair_scores_f64")
    got = bufs.get()
    bufs.free()
    if nq:
        assert got["Q"].tobytes() == Q.tobytes()
    if n:
        assert got["Y"].tobytes() == Y.tobytes()
    if npairs:
        assert np.array_equal(got["q"], pair_q) and np.array_equal(got["j"], pair_j)
    else:
        assert got["out"][0] == 7.5, "nothing is written without a pair"
    return got["out"][:npairs]


def rank_rows(ctx, Q, Y, id_base, tgt_ptr, tgt_score, tgt_id, splits=0, shift_q=0, shift_y=0, refused=None):
    """hnh_rank_rows_f64 with guard zones around every buffer and a workspace of exactly the size the library asks for; checks that the
    zones are intact and the inputs unchanged.  Returns the counts.  refused: the call must fail with that text in its message, and
    must have written nothing."""
    lib = K.load()
    (nq, R), n = Q.shape, Y.shape[0]
    tgt_ptr = np.ascontiguousarray(tgt_ptr, dtype=np.int64)  # (a HOST array)
    tgt_score, tgt_id = np.asarray(tgt_score, dtype=np.float64), np.asarray(tgt_id, dtype=np.int64)
    nt = len(tgt_score)
    need = lib.hnh_rank_rows_f64_workspace(nq, n, nt, splits)
    if refused is None:
        assert need >= 0 and need % 16 == 0
    bufs = Pack(ctx, Q=(Q if nq else np.zeros((1, R)), shift_q), Y=(Y if n else np.zeros((1, R)), shift_y), s=(tgt_score if nt else np.zeros(1), 0),
                i=(tgt_id if nt else np.zeros(1, np.int64), 0), counts=(np.full(max(nt, 1), UNTOUCHED, np.int64), 0))
    work = Scratch(ctx, max(need, 16))
    keep = tgt_ptr.copy()
    rc = lib.hnh_rank_rows_f64(ctx.h, bufs.ptr("Q"), nq, bufs.ptr("Y"), n, R, id_base, tgt_ptr.ctypes.data_as(C.c_void_p), bufs.ptr("s"), bufs.ptr("i"), splits,
                               bufs.ptr("counts"), work.ptr, max(need, 0), K.STREAM_COMPUTE)
    text = lib.hnh_last_error(ctx.h).decode() if rc != 0 else ""
    got = bufs.get()
    work.check()
    bufs.free()
    work.free()
    assert np.array_equal(tgt_ptr, keep)
    if nq:
        assert got["Q"].tobytes() == Q.tobytes()
    if n:
        assert got["Y"].tobytes() == Y.tobytes()
    if nt:
        assert got["s"].tobytes() == tgt_score.tobytes() and np.array_equal(got["i"], tgt_id)
    if refused is not None:
        assert rc != 0 and refused in text, (rc, text)
        assert np.all(got["counts"] == UNTOUCHED), "a refused call writes nothing"
        return None
    assert rc == 0, text
    if nt == 0:
        assert got["counts"][0] == UNTOUCHED, "nothing is written without a target"
    return got["counts"][:nt]


def rank_exclude(ctx, counts, excl_ptr, excl_score, excl_id, tgt_ptr, tgt_score, tgt_id):
    """hnh_rank_exclude_f64 between guard zones; returns the new counts"""
    lib = K.load()
    nq = len(tgt_ptr) - 1
    pad = lambda a, dt: np.asarray(a, dtype=dt) if len(a) else np.zeros(1, dt)  # noqa: E731
    arrays = dict(ep=(np.asarray(excl_ptr, np.int64), 0), es=(pad(excl_score, np.float64), 0), ei=(pad(excl_id, np.int64), 0),
                  tp=(np.asarray(tgt_ptr, np.int64), 0), ts=(pad(tgt_score, np.float64), 0), ti=(pad(tgt_id, np.int64), 0), counts=(pad(counts, np.int64), 0))
    bufs = Pack(ctx, **arrays)
    ctx.check(lib.hnh_rank_exclude_f64(ctx.h, nq, bufs.ptr("ep"), bufs.ptr("es"), bufs.ptr("ei"), bufs.ptr("tp"), bufs.ptr("ts"), bufs.ptr("ti"),
                                       bufs.ptr("counts"), K.STREAM_COMPUTE), "hnh_rank_exclude_f64")
    got = bufs.get()
    bufs.free()
    for name, (arr, _) in arrays.items():
        if name != "counts":
            assert got[name].tobytes() == arr.tobytes(), name
    return got["counts"][:len(counts)]


def targets_per_row(rng, nq, most):
    """tgt_ptr: `most` targets on every second row, a random number up to `most` on the others (most == 0: none anywhere)"""
    per = np.array([most if q % 2 == 0 else int(rng.integers(0, most + 1)) for q in range(nq)], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def mixed_targets(rng, S, id_base, tgt_ptr):
    """(tgt_score, tgt_id) for the integer-valued scores S [nq, n], taken in turn: a real item with its own score; a threshold half-way
    between two scores with an id from below, inside or above the range; the score of one item with the id of another (a tie that the
    id decides); and the row's previous target once more."""
    nq, n = S.shape
    score, ids = np.zeros(int(tgt_ptr[nq]) if nq else 0), np.zeros(int(tgt_ptr[nq]) if nq else 0, np.int64)
    for q in range(nq):
        for t in range(int(tgt_ptr[q]), int(tgt_ptr[q + 1])):
            kind = (t + q) % 4 if n else 1
            if kind == 3 and t > tgt_ptr[q]:
                score[t], ids[t] = score[t - 1], ids[t - 1]
            elif kind == 0 or kind == 3:
                j = int(rng.integers(0, n))
                score[t], ids[t] = S[q, j], id_base + j
            elif kind == 1:
                score[t] = (S[q, int(rng.integers(0, n))] if n else float(rng.integers(-3, 4))) + 0.5
                ids[t] = (5, id_base + int(rng.integers(0, n + 1)), id_base + n + 7)[int(rng.integers(0, 3))]
            else:
                score[t], ids[t] = S[q, int(rng.integers(0, n))], id_base + int(rng.integers(0, n))
    return score, ids
