"""ALS-CG through the operator on the HIP library against the numpy definition (tests/als_ref.py), ranks as loopback threads on one GPU:
every width class of the row kernels (one wave per row, wide rows, odd and non-power-of-two widths, the odd local widths of the R-split
schedules), a rectangular graph with hub rows on both sides (the folded CG epilogue as a launch of its own, S and S^T) and empty rows,
an R-MAT graph, three alternating steps (a held operand at an unchanged address with new contents), every schedule, the hold / ring /
chunk switches, and the built-in hashed set-up.  Same body as test_als_widths_cpu.py (tests/als_common.py); the bound is T.ALS_TOL, of
which the model's own rounding takes at most a tenth (test_als_model_cpu.py)."""
import pytest

import als_common as C
import hnh_testlib as T
from gat_gpu_harness import hip_backend  # noqa: F401

pytestmark = pytest.mark.gpu

SOLVER_CASES = C.gpu_solver_cases()
ARTIFICIAL_CASES = C.artificial_cases()


@pytest.mark.parametrize("case", SOLVER_CASES, ids=C.case_id)
def test_als_meets_the_model(case):
    C.run_case(*case)


@pytest.mark.parametrize("variant", C.VARIANTS, ids=lambda v: v[0])
def test_forced_steps_under_each_switch(monkeypatch, variant):
    """Forced mode (the longer one) at R = 128 on `hub` with the held operand switched off, the relay ring, separate CG updates, one mesh
    chunk, and the relay ring of two whose held block lives in the ring's spare buffer.  Each meets the model; how far holding moves the
    result (the window grouping changes the summation order) is recorded."""
    tag, alg, p, c, env = variant
    for k in ("HNH_NO_HOLD", "HNH_RING_MODE", "HNH_ALS_UNFOLDED", "HNH_MESH_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    base = C.RESULTS.get(("hub", 128, "forced", alg, p, c, "")) or C.run_case("hub", 128, "forced", alg, p, c)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = C.run_case("hub", 128, "forced", alg, p, c, tag=tag)
    diff = max(T.rel(got[k], base[k]) for k in got)
    T.record_observed("als_widths", graph="hub", R=128, mode="forced", alg=alg, p=p, c=c, variant=tag + " vs default", worst=diff)
    print("als_widths %s vs default: %.2e" % (tag, diff))
    assert diff <= 2 * T.ALS_TOL  # both within ALS_TOL of the same model


@pytest.mark.parametrize("case", ARTIFICIAL_CASES, ids=C.case_id)
def test_artificial_ground_truth_and_hashed_embeddings(case):
    C.run_artificial(*case)


def test_the_cases_are_the_ones_listed():
    """The table of cases: 15d_fusion2 at (1, 1) and (4, 1) over eleven widths in free mode and the forced widths (ten: R = 600 misses
    the float64 condition in forced mode, tests/golden/als_manifest.json "model_condition"), two R-MAT widths per mode, ten schedule grids
    x three widths per mode, five switches, five schedules x two widths of the built-in set-up.  Nothing is skipped: each is valid."""
    nforced = len(C.FORCED_WIDTHS)
    assert C.WIDTHS == (2, 8, 17, 32, 100, 128, 130, 256, 257, 384, 600) and C.FORCED_WIDTHS in (C.WIDTHS, C.WIDTHS[:-1])
    assert len(SOLVER_CASES) == len(set(SOLVER_CASES)) == 2 * 11 + 2 * nforced + 2 * 2 + 2 * 10 * 3
    assert len(C.VARIANTS) == 5 and len(ARTIFICIAL_CASES) == len(set(ARTIFICIAL_CASES)) == 10
    for g, R, mode, alg, p, c in SOLVER_CASES:
        assert T.valid_config(alg, p, c, R)
    # the R-split schedules' local widths at the three schedule widths
    assert [R // 4 for R in C.SCHEDULE_WIDTHS] == [2, 25, 64]
