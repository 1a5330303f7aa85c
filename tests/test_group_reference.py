"""CPU: the longdouble reference of the group-selection kernels (tests/groupref.py) and its bounds.  fp64 NumPy evaluating the
kernels' formulas in both forms (eigh-sqrtm and Cholesky) sits inside every bound -- that is where the constants come from
-- every assert_* helper fails on a result wrong at 1e-9 relative, and stand-ins of the defects tests/test_group_ops_gpu.py
exists for fail their helper."""
import numpy as np
import pytest

import glmref
import groupref as R
import xprec

pytestmark = pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format")


@pytest.fixture(scope="module")
def wide():
    """A well-conditioned call with groups past GRP_MAX, w1, w2, lam > 0 and non-zero beta (lm = 0), with its reference."""
    case = R.make_case(R.WIDTHS[40], 257, 20)
    assert not case["lm"] and case["w1"] is not None and case["w2"] is not None and case["lam"] > 0 and case["beta"].any()
    mom = R.moments(case)
    return case, mom, R.scores(case, mom)


@pytest.fixture(scope="module")
def lm_case():
    """An LM call (n_t != n, three row blocks, lam > 0, non-zero beta) on the <8> template."""
    case = R.make_case(R.WIDTHS[8], 257, 15)
    assert case["lm"] and case["n_t"] != 257 and case["part"].shape[0] == 3 and case["lam"] > 0 and case["beta"].any()
    mom = R.moments(case)
    return case, mom, R.scores(case, mom)


def test_the_hand_written_cholesky_solves():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((60, 23))
    M = R.ld(A.T @ A)
    L = R.chol(M)
    assert float(np.abs(L @ L.T - M).max()) < 1e-16 * float(np.abs(M).max())
    b = R.ld(rng.standard_normal(23))
    x = R.bwd(L, R.fwd(L, b))
    assert float(np.abs(M @ x - b).max()) < 1e-15
    assert np.allclose(x.astype(np.float64), np.linalg.solve(A.T @ A, b.astype(np.float64)), rtol=1e-9)


def test_the_cases_cover_what_the_kernels_branch_on():
    cases = R.all_score_cases()
    widths = set(s for c in cases.values() for s in c["widths"])
    assert {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 24, 25, 29, 40} <= widths
    assert {c["X"].shape[0] for c in cases.values()} >= set(R.ROWS)
    assert {len(c["widths"]) for c in cases.values()} >= set(R.GROUP_COUNTS)
    for smax in R.WIDTHS:
        mine = [c for c in cases.values() if max(c["widths"]) == smax]
        for key, values in (("lm", (False, True)), ("lam", (0.0, 0.05))):
            assert {c[key] for c in mine} >= set(values), (smax, key)
        for key in ("w1", "w2", "always"):
            assert {c[key] is None for c in mine} == {False, True}, (smax, key)
        assert {bool(c["beta"].any()) for c in mine} == {False, True}, smax
        assert any(not c["lm"] and c["w2"] is None for c in mine), (smax, "dcol left untouched and used as d")
        assert any(not c["lm"] and c["w2"] is not None for c in mine), (smax, "dcol from the moment pass")
        assert {c["part"].shape[0] for c in mine if c["lm"]} == {1, 3}, smax
        assert all(c["n_t"] != c["X"].shape[0] for c in mine if c["lm"]), smax
    assert any(c["X"].shape[0] < max(c["widths"]) and c["lam"] > 0 for c in cases.values())


def test_fp64_numpy_sits_inside_every_bound_and_fixes_the_constants():
    worst = {"moments": (0.0, ""), "dcol": (0.0, ""), "score eigh": (0.0, ""), "score chol": (0.0, ""), "lsq chol": (0.0, ""),
             "lsq solve": (0.0, "")}

    def note(key, value, name):
        if value > worst[key][0]:
            worst[key] = (value, name)

    cmax = 0.0
    for name, case in R.all_score_cases().items():
        mom = R.moments(case)
        sref = R.scores(case, mom)
        cmax = max(cmax, float(sref["cond"].max()))
        blocks, dcol = R.moments_fp64(case)
        note("moments", R.assert_moments_close(blocks, mom, name), name)
        note("dcol", R.assert_dcol_close(dcol, case, mom, name), name)
        for form in ("eigh", "chol"):
            bd = R.scores_fp64(case, blocks, dcol, form)
            note("score " + form, R.score_units(bd, sref)[0], name)
            R.assert_scores_close(bd, sref, name + " " + form)
    for n, (X, gidx, yw, drop) in [(n, R.lsq_case(n)) for n in R.LSQ_ROWS] + [(3, R.lsq_short_case())]:
        ref = R.lsq(X, gidx, yw, drop)
        for form in ("chol", "solve"):
            got = R.lsq_fp64(X, gidx, yw, form, drop)
            note("lsq " + form, R.lsq_units(got, ref)[0], "n=%d" % n)
            R.assert_lsq_close(got, ref, "lsq n=%d %s" % (n, form))
    for key, (value, name) in worst.items():
        print("fp64 NumPy, %s: %.4f of the bound at c = 1 (%s)" % (key, value, name))
    print("largest cond_2(M_g) of the cases: %.3g (limit %g)" % (cmax, R.COND_LIMIT))
    score = max(worst["score eigh"][0], worst["score chol"][0])
    lsq = max(worst["lsq chol"][0], worst["lsq solve"][0])
    # the rule of the issue, written out: the next power of two at or above four times the maximum, no floor
    assert abs(score - R.SCORE_NUMPY_MAX) <= 5e-4 and R.SCORE_C == 2.0 ** np.ceil(np.log2(4 * R.SCORE_NUMPY_MAX)), score
    assert abs(lsq - R.LSQ_NUMPY_MAX) <= 5e-4 and R.LSQ_C == 2.0 ** np.ceil(np.log2(4 * R.LSQ_NUMPY_MAX)), lsq
    assert R.constant_from is glmref.constant_from
    assert abs(worst["moments"][0] - R.MOMENT_NUMPY_MAX) <= 5e-4, worst["moments"]
    assert abs(worst["dcol"][0] - R.DCOL_NUMPY_MAX) <= 5e-4, worst["dcol"]
    assert cmax <= R.COND_LIMIT


def test_every_helper_fails_on_a_result_wrong_at_1e_9(wide, lm_case):
    for case, mom, sref in (wide, lm_case):
        blocks, dcol = R.moments_fp64(case)
        bd = R.scores_fp64(case, blocks, dcol, "chol")
        R.assert_moments_close(blocks, mom, "intact")
        R.assert_dcol_close(dcol, case, mom, "intact")
        R.assert_scores_close(bd, sref, "intact")
        g = len(blocks) - 3
        s = blocks[g].shape[0]
        for u, v in ((0, 0), (s - 1, 0), (s - 1, s - 1)):
            bad = [b.copy() for b in blocks]
            bad[g][u, v] = bad[g][v, u] = bad[g][u, v] * (1 + 1e-9)
            with pytest.raises(AssertionError):
                R.assert_moments_close(bad, mom, "an entry off by 1e-9")
        bad = [b.copy() for b in blocks]
        bad[g][s - 1, 0] = np.nextafter(bad[g][s - 1, 0], np.inf)
        with pytest.raises(AssertionError, match="symmetric"):
            R.assert_moments_close(bad, mom, "one ulp of asymmetry")
        for j in (0, dcol.size - 1):
            bad = dcol.copy()
            bad[j] *= 1 + 1e-9
            with pytest.raises(AssertionError):
                R.assert_dcol_close(bad, case, mom, "dcol off by 1e-9")
        for j in range(bd.size):
            bad = bd.copy()
            bad[j] *= 1 + 1e-9
            with pytest.raises(AssertionError):
                R.assert_scores_close(bad, sref, "a score off by 1e-9")
            bad[j] = np.nan
            with pytest.raises(AssertionError):
                R.assert_scores_close(bad, sref, "a NaN score")
    X, gidx, yw, drop = R.lsq_case(257)
    ref = R.lsq(X, gidx, yw, drop)
    got = R.lsq_fp64(X, gidx, yw, "chol", drop)
    R.assert_lsq_close(got, ref, "intact")
    for j in range(got.size):
        bad = got.copy()
        bad[j] = bad[j] * (1 + 1e-9) if np.isfinite(bad[j]) else np.nan
        with pytest.raises(AssertionError):
            R.assert_lsq_close(bad, ref, "an lsq score off by 1e-9, or NaN for +inf")


def test_an_ill_conditioned_group_is_refused_not_skipped():
    case = R.make_case(R.WIDTHS[4], 257, 0, noise=1e-7)
    sref = R.scores(case)
    assert sref["cond"].max() > R.COND_LIMIT
    with pytest.raises(AssertionError, match="ill-conditioned"):
        R.assert_scores_close(sref["bd"].astype(np.float64), sref, "noise 1e-7")


# ---- stand-ins of the defects the GPU file exists for -------------------------------------------------------------------------
@pytest.mark.parametrize("n", (255, 257, 1000))
def test_defect_last_two_rows_dropped_from_a_moment(n):
    for smax in R.WIDTHS:
        case = R.make_case(R.WIDTHS[smax], n, 4)
        mom = R.moments(case)
        R.assert_moments_close(R.moments_fp64(case)[0], mom, "intact")
        blocks, dcol = R.moments_fp64(case, drop_rows=[n - 1, n - 2])
        with pytest.raises(AssertionError):
            R.assert_moments_close(blocks, mom, "rows n-1, n-2 dropped")
        with pytest.raises(AssertionError):
            R.assert_dcol_close(dcol, case, mom, "rows n-1, n-2 dropped")


@pytest.mark.parametrize("g,tu,tv", ((6, 4, 2), (6, 3, 3), (2, 2, 0), (4, 3, 1)))
def test_defect_one_tile_of_a_wide_block_zero_or_transposed(wide, g, tu, tv):
    case, mom, _ = wide
    assert case["widths"][g] > R.GRP_MAX and tu * R.TILE < case["widths"][g]
    with pytest.raises(AssertionError):
        R.assert_moments_close(R.moments_fp64(case, zero_tile=(g, tu, tv))[0], mom, "a tile left at zero")
    if tu != tv and (tu + 1) * R.TILE <= case["widths"][g]:
        with pytest.raises(AssertionError):
            R.assert_moments_close(R.moments_fp64(case, transpose_tile=(g, tu, tv))[0], mom, "a tile transposed")


def test_defect_n_t_division_omitted_from_d(lm_case):
    case, _, sref = lm_case
    blocks, dcol = R.moments_fp64(case)
    with pytest.raises(AssertionError):
        R.assert_scores_close(R.scores_fp64(case, blocks, dcol, "eigh", nt_in_d=False), sref, "d not divided by n_t")


@pytest.mark.parametrize("ridge", ("all", "none"))
def test_defect_ridge_off_the_diagonal_or_omitted(wide, lm_case, ridge):
    for case, _, sref in (wide, lm_case):
        blocks, dcol = R.moments_fp64(case)
        for form in ("eigh", "chol"):
            with pytest.raises(AssertionError):
                R.assert_scores_close(R.scores_fp64(case, blocks, dcol, form, ridge=ridge), sref, "ridge " + ridge)


def test_defect_score_divided_by_grp_max(lm_case):
    case, _, sref = lm_case
    blocks, dcol = R.moments_fp64(case)
    with pytest.raises(AssertionError):
        R.assert_scores_close(R.scores_fp64(case, blocks, dcol, "eigh", divide_by=R.GRP_MAX), sref, "divided by GRP_MAX")


def test_defect_stored_eigenvectors_of_another_group():
    case = R.make_case((5, 5, 3, 3, 9, 9), 257, 3)
    sref = R.scores(case)
    blocks, dcol = R.moments_fp64(case)
    R.assert_scores_close(R.scores_fp64(case, blocks, dcol, "eigh"), sref, "intact")
    for g, other in ((0, 1), (3, 2), (5, 4)):
        with pytest.raises(AssertionError):
            R.assert_scores_close(R.scores_fp64(case, blocks, dcol, "eigh", eig_from={g: other}), sref, "stale eigenvectors")


def test_defect_dcol_indexed_by_panel_column_under_cshift():
    case = R.panel_case()
    mom = R.moments(case)
    panel, cs = R.panel_of(case)
    assert cs > 0 and panel["X"].shape[1] == case["X"].shape[1] - cs
    shifted = dict(case, X=np.concatenate([np.zeros((case["X"].shape[0], cs)), panel["X"]], axis=1))
    blocks, dcol = R.moments_fp64(shifted, cshift=cs)
    assert blocks[2] is None and blocks[3] is not None
    R.assert_moments_close(blocks, mom, "panel", only=range(3, len(blocks)))
    R.assert_dcol_close(dcol, case, mom, "panel", lo=cs)
    with pytest.raises(AssertionError):
        R.assert_dcol_close(R.moments_fp64(shifted, cshift=cs, panel_dcol=True)[1], case, mom, "panel index", lo=cs)
