"""The top-k kernels of include/hnh_topk.h where tests/test_als_topk_gpu.py does not look.  Every comparison is array_equal against the
numpy definition (tests/als_topk_ref.py) on operands whose scores are exact integers, or bytes against splits = 1; no tolerance anywhere.
Every device buffer lies between guard zones (als_topk_common.Guarded) and the inputs come back unchanged.

Hostile item orders (als_topk_common.ordered_case; tests/test_als_topk_cpu.py shows on the CPU which cuts of the candidate buffer they
force): every tile passes for every row, nothing passes after the first cut, all ties, one item per tile; at k on both sides of the switch
of the buffer's size (64 / 65), with and without lists, splits 1 and 3.
Widths and geometry on random integers: R in {1, 3, 4, 12, 16, 124, 132, 500} (16-byte loads with one lane group in four, exactly one K
tile, a partial last K tile without Q in registers), k in {63, 64, 65, 127}, nq in {128, 129, 300} (a second and third workgroup in x), n
in {64, 129, 1000}.
Bases that are only 8-byte aligned with R % 4 == 0 (the 8-byte instance where the 16-byte one is the usual): the same bytes.
Many splits: 9 .. 1024 forced, with a workspace of exactly the size the refused call names; two merge levels above 32; ranges of one item
and empty ranges.  The library's own choice above the merge fan (asserted > 32).
The merge with 31 .. 300 lists, whole parts empty (the first too), NaN as the score of empty entries, -0.0 against +0.0.
Refusals by message, id_base outside [0, INT64_MAX - n] among them; Y == NULL with n == 0 is accepted."""
import functools

import numpy as np
import pytest

import als_common
import als_topk_common as TC
import als_topk_ref as TR
from als_topk_common import Guarded, integers, random_lists, topk_merge, topk_rows
from distributed_sddmm_amd import _kernels as K
from gat_gpu_harness import ctx, hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu

# (nq, n, R, k).  16640 items = 260 tiles: the buffer creeps to its cap one item a tile and is cut there (tests/test_als_topk_cpu.py)
ORDER_SHAPES = [(33, 16640, 4, 10), (33, 16640, 3, 64), (17, 16640, 16, 65), (33, 16640, 132, 100), (33, 2000, 1, 127), (33, 2000, 12, 128)]
ORDER_CASES = [(kind,) + shape for shape in ORDER_SHAPES for kind in TC.KINDS if not (kind == "trickle" and shape[1] == 2000)]
WIDE_RS, WIDE_KS, WIDE_NQS, WIDE_NS = (1, 3, 4, 12, 16, 124, 132, 500), (63, 64, 65, 127), (128, 129, 300), (64, 129, 1000)
WIDE_CASES = [(128, 64, 1, 63), (129, 129, 3, 64), (300, 1000, 4, 65), (128, 1000, 12, 127), (129, 64, 16, 65), (300, 129, 124, 64),
              (129, 1000, 132, 63), (128, 129, 500, 127), (300, 64, 132, 127), (129, 1000, 500, 65)]
MANY_SPLITS = (9, 32, 33, 64, 1024)
MERGE_CASES = [(parts, k) for parts in (31, 32, 33, 100) for k in (1, 10, 85, 128)] + [(300, 1)]
INT64_MAX = 2**63 - 1


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_the_cases_are_the_ones_listed():
    assert len(ORDER_CASES) == len(set(ORDER_CASES)) == 22
    assert {c[0] for c in ORDER_CASES if c[2] == 16640} == set(TC.KINDS) and {c[0] for c in ORDER_CASES if c[2] == 2000} == set(TC.KINDS) - {"trickle"}
    assert {c[1:] for c in ORDER_CASES} == {(33, 16640, 4, 10), (33, 16640, 3, 64), (17, 16640, 16, 65), (33, 16640, 132, 100), (33, 2000, 1, 127),
                                            (33, 2000, 12, 128)}
    assert len(WIDE_CASES) == len(set(WIDE_CASES)) <= 12
    assert {c[0] for c in WIDE_CASES} == set(WIDE_NQS) == {128, 129, 300} and {c[1] for c in WIDE_CASES} == set(WIDE_NS) == {64, 129, 1000}
    assert {c[2] for c in WIDE_CASES} == set(WIDE_RS) == {1, 3, 4, 12, 16, 124, 132, 500} and {c[3] for c in WIDE_CASES} == set(WIDE_KS) == {63, 64, 65, 127}
    assert any(R > 128 and R % 4 == 0 and R % 16 for _, _, R, _ in WIDE_CASES), "Q re-read per tile, 16-byte loads, a partial last K tile"
    assert MANY_SPLITS == (9, 32, 33, 64, 1024) and K.TOPK_MAX_SPLITS == 1024
    assert set(MERGE_CASES) == {(p, k) for p in (31, 32, 33, 100) for k in (1, 10, 85, 128)} | {(300, 1)} and len(MERGE_CASES) == 17
    assert all((256 - k) // k < parts for parts, k in MERGE_CASES if k > 1) and (256 - 1) // 1 < 300, "more lists than one round holds"


# ------------------------------------------------------------------------------------------------ hostile orders
@pytest.mark.parametrize("case", ORDER_CASES, ids=als_common.case_id)
def test_hostile_item_orders_equal_the_definition(ctx, case):
    kind, nq, n, R, k = case
    Q, Y = TC.ordered_case(kind, nq, n, R)
    rng = np.random.default_rng(n + R + k)
    for excluded in (None, random_lists(rng, nq, n)):
        want_ids, want_scores = TR.topk(Q, Y, k, 7, excluded)
        for splits in (1, 3):
            ids, scores = topk_rows(ctx, Q, Y, k, 7, excluded, splits)
            assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores), (excluded is not None, splits)


# ------------------------------------------------------------------------------------------------ widths and geometry
@pytest.mark.parametrize("case", WIDE_CASES, ids=als_common.case_id)
def test_widths_and_geometry_are_exact_on_integers(ctx, case):
    nq, n, R, k = case
    rng = np.random.default_rng(list(case))
    Q, Y = integers(rng, (nq, R)), integers(rng, (n, R))
    for excluded in (None, random_lists(rng, nq, n)):
        want_ids, want_scores = TR.topk(Q, Y, k, 10**10, excluded)
        ids, scores = topk_rows(ctx, Q, Y, k, 10**10, excluded)
        assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores)


@pytest.mark.parametrize("R", [8, 256])
def test_bases_aligned_to_8_bytes_give_the_same_bytes(ctx, R):
    nq, n, k = 33, 1000, 10
    rng = np.random.default_rng(R)
    Q, Y = rng.standard_normal((nq, R)), rng.standard_normal((n, R))
    excluded = random_lists(rng, nq, n)
    aligned = topk_rows(ctx, Q, Y, k, 0, excluded, 1)
    for shifts in (dict(shift_q=8), dict(shift_y=8), dict(shift_q=8, shift_y=8), dict(shift_out=8), dict(shift_q=8, shift_y=8, shift_out=8)):
        for splits in (1, 2):
            assert same(topk_rows(ctx, Q, Y, k, 0, excluded, splits, **shifts), aligned), (shifts, splits)


# ------------------------------------------------------------------------------------------------ many splits
@pytest.mark.parametrize("R", [8, 256])
@pytest.mark.parametrize("nq,n", [(5, 65), (70, 5000)])
def test_many_forced_splits_give_the_bytes_of_one(ctx, nq, n, R):
    lib = K.load()
    k = 10
    rng = np.random.default_rng(nq + n + R)
    Q, Y = rng.standard_normal((nq, R)), rng.standard_normal((n, R))
    excluded = random_lists(rng, nq, n)
    first = topk_rows(ctx, Q, Y, k, 0, excluded, 1)
    documented = lib.hnh_topk_rows_f64_workspace(nq, n, R, k)
    for splits in MANY_SPLITS:
        ids, scores, said = topk_rows(ctx, Q, Y, k, 0, excluded, splits, exact_work=True)  # (the guards of the exact workspace: in topk_rows)
        assert said == splits
        assert same((ids, scores), first), splits
    # more than 8 forced splits need more than the documented size, and the call says so instead of running
    q, y, out, work = (Guarded(ctx, a) for a in (Q, Y, np.full((nq, k), 7.5), np.zeros(documented, np.uint8)))
    rc = lib.hnh_topk_rows_f64(ctx.h, q.ptr, nq, y.ptr, n, R, 0, None, None, k, 9, out.ptr, out.ptr, work.ptr, documented, K.STREAM_COMPUTE)
    assert rc == 1 and b"the workspace is too small: %d bytes" % documented in lib.hnh_last_error(ctx.h) and b"needed with 9 splits" in lib.hnh_last_error(ctx.h)
    assert np.all(out.get() == 7.5) and np.all(work.get() == 0), "nothing is launched"
    for b in (q, y, out, work):
        b.free()


@functools.lru_cache(maxsize=None)
def own_choice_case():
    """129 integer queries on 81920 items and their first 128 by the definition, computed once (a query's list depends on its own row
    only, so the first 5 queries are a case too, and the first 10 entries are the answer at k = 10: the order is strict)"""
    rng = np.random.default_rng(129)
    Q, Y = integers(rng, (129, 8)), integers(rng, (81920, 8))
    excluded = random_lists(rng, 129, 81920)
    want = TR.topk(Q, Y, 128, 3, excluded)
    for a in (Q, Y) + want:
        a.setflags(write=False)
    return Q, Y, excluded, want


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("nq", [5, 129])
def test_the_librarys_own_choice_above_the_merge_fan(ctx, nq, k):
    Q, Y, excluded, want = own_choice_case()
    Q, excluded, want = Q[:nq], excluded[:nq], (want[0][:nq], want[1][:nq])
    ids, scores, said = topk_rows(ctx, Q, Y, k, 3, excluded, 0, exact_work=True)
    assert said > 32, "the library's own choice no longer takes the two-level merge: this test has lost what it is for"
    assert np.array_equal(ids, want[0][:, :k]) and np.array_equal(scores, want[1][:, :k])
    assert same(topk_rows(ctx, Q, Y, k, 3, excluded, 1), (ids, scores))
    assert same(topk_rows(ctx, Q, Y, k, 3, excluded, 0), (ids, scores)), "with the documented workspace size too"


# ------------------------------------------------------------------------------------------------ merge
def cut_lists(Q, Y, k, cuts, id_base):
    lists = [TR.topk(Q, Y[a:b], k, id_base + a) for a, b in zip(cuts[:-1], cuts[1:])]
    in_i, in_s = np.stack([x[0] for x in lists]), np.stack([x[1] for x in lists])
    in_s[in_i == -1] = np.nan  # the score of an empty entry is ignored
    return in_s, in_i


@pytest.mark.parametrize("parts,k", MERGE_CASES)
def test_merge_of_many_lists_reproduces_the_whole(ctx, parts, k):
    nq, R = 17, 8
    rng = np.random.default_rng(parts * 1000 + k)
    # fewer items than parts: whole parts are empty ...
    n = parts - 7
    Q, Y = integers(rng, (nq, R)), integers(rng, (n, R))
    cuts = np.linspace(0, n, parts + 1).astype(int)
    in_s, in_i = cut_lists(Q, Y, k, cuts, 1000)
    assert np.sum(np.all(in_i == -1, axis=(1, 2))) >= 7 and np.isnan(in_s).any()
    ids, scores = topk_merge(ctx, in_s, in_i, k)
    want_ids, want_scores = TR.topk(Q, Y, k, 1000)
    assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores)
    # ... and enough items that every round of the merge drops some, in parts of uneven length, the first one and others empty
    n = 12 * parts + 3 * k
    Q, Y = integers(rng, (nq, R)), integers(rng, (n, R))
    cuts = np.sort(np.concatenate([[0, 0, n], rng.integers(0, n + 1, parts - 2)]))
    cuts[rng.integers(2, parts, 3)] = cuts[rng.integers(2, parts, 3)]
    cuts = np.sort(cuts)
    assert len(cuts) == parts + 1 and cuts[0] == cuts[1] == 0 and cuts[-1] == n
    in_s, in_i = cut_lists(Q, Y, k, cuts, 0)
    assert np.all(in_i[0] == -1) and np.all(np.isnan(in_s[0])), "the first part is empty"
    ids, scores = topk_merge(ctx, in_s, in_i, k)
    want_ids, want_scores = TR.topk(Q, Y, k, 0)
    assert np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores)
    assert np.all(ids[:, :min(k, n)] >= 0)


def test_merge_keeps_the_sign_of_a_zero_and_orders_zeros_by_id(ctx):
    k, e = 6, (np.nan, -1)
    parts = [[(1.0, 9), (-0.0, 5), (-1.0, 11), e, e, e],
             [(0.0, 2), (-0.0, 7), (-2.0, 1), e, e, e],
             [e, e, e, e, e, e],
             [(0.0, 3), (-0.0, 4), (0.0, 8), (-5.0, 0), e, e]]
    in_s = np.array([[[c[0] for c in p]] for p in parts])
    in_i = np.array([[[c[1] for c in p]] for p in parts], dtype=np.int64)
    ids, scores = topk_merge(ctx, in_s, in_i, k)
    assert ids.tolist() == [[9, 2, 3, 4, 5, 7]], "zeros tie whatever their sign and come out by ascending id"
    assert scores.tobytes() == np.array([[1.0, 0.0, 0.0, -0.0, -0.0, -0.0]]).tobytes(), "each with the bits it went in with"
    # all ten real entries, in the total order, then the empty tail
    wide_s, wide_i = np.full((4, 1, 12), np.nan), np.full((4, 1, 12), -1, dtype=np.int64)
    wide_s[:, :, :6], wide_i[:, :, :6] = in_s, in_i
    ids, scores = topk_merge(ctx, wide_s, wide_i, 12)
    assert ids.tolist() == [[9, 2, 3, 4, 5, 7, 8, 11, 1, 0, -1, -1]]
    assert scores.tobytes() == np.array([[1.0, 0.0, 0.0, -0.0, -0.0, -0.0, 0.0, -1.0, -2.0, -5.0, -np.inf, -np.inf]]).tobytes()


# ------------------------------------------------------------------------------------------------ refusals
def test_more_refusals_by_message(ctx):
    lib = K.load()
    nq, n, R, k = 4, 8, 8, 10
    wb = 1 << 20
    bufs = dict(q=Guarded(ctx, np.zeros((nq, R))), y=Guarded(ctx, np.zeros((n, R))), s=Guarded(ctx, np.full((nq, 128), 7.5)),
                i=Guarded(ctx, np.full((nq, 128), -7, np.int64)), work=Guarded(ctx, np.zeros(wb + 16, np.uint8)), ptr=Guarded(ctx, np.zeros(nq + 1, np.int64)))
    q, y, s, i, work, ptr = (bufs[name].ptr for name in ("q", "y", "s", "i", "work", "ptr"))

    def rows(text, n=n, id_base=0, excl_ptr=None, excl_idx=None, splits=0, work=work, y=y, status=1):
        rc = lib.hnh_topk_rows_f64(ctx.h, q, nq, y, n, R, id_base, excl_ptr, excl_idx, k, splits, s, i, work, wb, K.STREAM_COMPUTE)
        assert rc == status and text in lib.hnh_last_error(ctx.h), (rc, lib.hnh_last_error(ctx.h))

    rows(b"splits must be between 0 and HNH_TOPK_MAX_SPLITS = 1024", splits=-1)
    rows(b"splits must be between 0 and HNH_TOPK_MAX_SPLITS = 1024", splits=1025)
    rows(b"the workspace must be 16-byte aligned", work=work + 8)
    rows(b"null pointer", excl_ptr=ptr, excl_idx=None)
    rows(b"null pointer", y=None)
    # -1 is the empty entry and the merge takes every negative id for one: ids are id_base .. id_base + n - 1 and must be real
    for splits in (1, 2):
        rows(b"id_base", id_base=-3, splits=splits)
        rows(b"id_base", id_base=-1, splits=splits)
        rows(b"id_base", id_base=INT64_MAX - n + 1, splits=splits)
        rows(b"id_base", id_base=INT64_MAX, splits=splits)
    for fn, args, text in ((lib.hnh_topk_merge_f64, (s, i, 0, nq, k, s, i), b"parts < 1"),
                           (lib.hnh_topk_merge_f64, (s, i, 2, nq, 129, s, i), b"k must be between 1 and HNH_TOPK_MAX_K = 128"),
                           (lib.hnh_topk_merge_f64, (s, None, 2, nq, k, s, i), b"null pointer"),
                           (lib.hnh_topk_merge_f64, (s, i, 2, nq, k, None, i), b"null pointer"),
                           (lib.hnh_take_rows_f64, (q, nq, 0, i, nq, s), b"R < 1")):
        rc = fn(ctx.h, *args, K.STREAM_COMPUTE)
        assert rc == 1 and text in lib.hnh_last_error(ctx.h), lib.hnh_last_error(ctx.h)
    got = {name: b.get() for name, b in bufs.items()}
    assert np.all(got["s"] == 7.5) and np.all(got["i"] == -7) and np.all(got["work"] == 0), "a refused call launches nothing"
    # the largest id_base that is allowed, at both split counts; without items Y may be NULL and every entry is empty
    Q, Y = integers(np.random.default_rng(0), (nq, R)), integers(np.random.default_rng(1), (n, R))
    want = TR.topk(Q, Y, k, INT64_MAX - n)
    for splits in (1, 2):
        ids, scores = topk_rows(ctx, Q, Y, k, INT64_MAX - n, None, splits)
        assert np.array_equal(ids, want[0]) and np.array_equal(scores, want[1]) and ids.max() == INT64_MAX - 1
    for splits in (0, 1, 5):
        out_s, out_i = Guarded(ctx, np.full((nq, k), 7.5)), Guarded(ctx, np.full((nq, k), -7, np.int64))
        ctx.check(lib.hnh_topk_rows_f64(ctx.h, q, nq, None, 0, R, 0, None, None, k, splits, out_s.ptr, out_i.ptr, work, wb, K.STREAM_COMPUTE),
                  "Y == NULL with n == 0")
        assert np.all(out_i.get() == -1) and np.all(out_s.get() == -np.inf), splits
        out_s.free(); out_i.free()
    for b in bufs.values():
        b.free()
