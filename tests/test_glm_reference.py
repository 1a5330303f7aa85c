"""CPU: the longdouble reference of the logistic and Poisson solver kernels (tests/glmref.py) against fp64 NumPy on every
case of tests/test_glm_ops_gpu.py.  fp64 NumPy sits inside every bound (this is where the constants of the bounds are
measured); every helper fails on a result that is wrong at 1e-9 in one entry; NumPy stand-ins of the defects the GPU file
exists to catch fail the helper they should, on the GPU file's own small shapes; the constructed cases are what their
docstrings say."""
import numpy as np
import pytest

import glmref as R
import xprec
from bess_amd import capi

pytestmark = pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format here")

def _up(worst, key, value, what):
    if value > worst.get(key, (-1.0, ""))[0]:
        worst[key] = (value, what)


def _check_constants(worst, keys):
    for k in keys:
        measured, where = worst[k]
        stored, c = (R.ROW_NUMPY_MAX[k], R.ROW_C[k]) if k in R.ROW_C else {"sum": (R.SUM_NUMPY_MAX, R.SUM_C), "score": (R.SCORE_NUMPY_MAX, R.SCORE_C)}[k]
        print("fp64 NumPy %s: %.4f of the first-order bound at %s (recorded %.4f, constant %g)" % (k, measured, where, stored, c))
        assert measured <= stored * 1.0000001, (k, measured, stored, where)  # the recorded maximum covers the measured one
        assert c == R.constant_from(stored), (k, c, R.constant_from(stored))


# ---- fp64 NumPy inside every bound; the constants ---------------------------------------------------------------------------
def test_fp64_numpy_gh_sits_inside_every_bound_and_fixes_the_constants():
    worst = {}
    for name, (family, case, lam) in R.all_gh_cases().items():
        X, y, w, mk, cols, b, coef0 = case
        ref, got = R.gh(family, *case), R.gh_fp64(family, *case)
        _up(worst, "g", R.row_units(got["g"], ref["g"], ref["dg"])[0], name)
        _up(worst, "h", R.row_units(got["h"], ref["h"], ref["dh"])[0], name)
        _up(worst, "sum", R.sum_units(got["loss"][0], ref["loss_all"], ref["loss_all_bound"]), name + " loss")
        _up(worst, "sum", R.sum_units(got["loss"][1], ref["loss_test"], ref["loss_test_bound"]), name + " held-out loss")
        sref = R.scores(X, ref, cols, b, lam)
        assert np.isfinite(sref["bd"].astype(np.float64)).all() and (sref["l2"] > 0).all(), name  # no column is left out
        _up(worst, "score", R.score_units(R.scores_fp64(X, got["g"], got["h"], cols, b, lam), sref)[0], name)
        R.assert_g_close(got["g"], ref, name)
        R.assert_h_close(got["h"], ref, name)
        R.assert_loss_close(got["loss"][0], ref, name)
        R.assert_loss_close(got["loss"][1], ref, name, test=True)
        R.assert_scores_close(R.scores_fp64(X, got["g"], got["h"], cols, b, lam), sref, name)
    _check_constants(worst, ("g", "h", "score"))
    assert worst["sum"][0] <= R.SUM_NUMPY_MAX * 1.0000001, worst["sum"]


def test_fp64_numpy_irls_sits_inside_every_bound_and_fixes_the_constants():
    worst, solved = {}, {}
    for name, (family, case, t, wfloor, lam) in R.all_irls_cases().items():
        ref, got = R.irls(family, *case, t, wfloor), R.irls_fp64(family, *case, t, wfloor, lam)
        _up(worst, "wv", R.row_units(got["wv"], ref["wv"], ref["dwv"])[0], name)
        _up(worst, "z", R.row_units(got["z"], ref["z"], ref["dz"])[0], name)
        _up(worst, "sum", R.sum_units(got["ll"], ref["ll"], ref["ll_bound"]), name + " ll")
        R.assert_wv_close(got["wv"], ref, name)
        R.assert_z_close(got["z"], ref, name)
        R.assert_ll_close(got["ll"], ref, name)
        R.assert_gram_close(got["gram"], ref, name)
        # (the systems of (a) and (b) are not solved: some have more unknowns than rows; beside a saturated Poisson row the
        # condition number is past 1e13 and assert_bnext_close itself refuses the case)
        if name.startswith("s ") or name.startswith("c fam%d" % R.LOGISTIC):
            R.assert_bnext_close(got["bnext"], ref, lam, name)
            solved[family] = solved.get(family, 0) + 1
        elif name.startswith("c "):
            assert R.next_iterate(ref, lam)[1] > 1e12
            with pytest.raises(AssertionError):
                R.assert_bnext_close(got["bnext"], ref, lam, name)
    _check_constants(worst, ("wv", "z", "sum"))
    assert solved[R.POISSON] == 2 * len(R.SOLVE_CASES) and solved[R.LOGISTIC] == solved[R.POISSON] + 9, solved


# ---- every helper fails at 1e-9 ---------------------------------------------------------------------------------------------
def _bump(a, i):
    a = np.array(a, dtype=np.float64)
    a[i] *= 1.0 + 1e-9
    return a


@pytest.mark.parametrize("family", (R.LOGISTIC, R.POISSON))
def test_every_helper_fails_on_a_result_that_is_wrong_at_1e_9_in_one_entry(family):
    case = R.gh_case(family, 1025, 17, "wide", True, True)
    X, y, w, mk, cols, b, coef0 = case
    ref, good = R.gh(family, *case), R.gh_fp64(family, *case)
    i = int(np.argmax(np.abs(good["g"]) * (good["h"] > 0)))
    sref = R.scores(X, ref, cols, b, 0.05)
    bd = R.scores_fp64(X, good["g"], good["h"], cols, b, 0.05)
    for helper, ok, bad in (
            (R.assert_g_close, good["g"], _bump(good["g"], i)), (R.assert_h_close, good["h"], _bump(good["h"], i)),
            (R.assert_loss_close, good["loss"][0], good["loss"][0] * (1 + 1e-9))):
        helper(ok, ref, "unperturbed")
        with pytest.raises(AssertionError):
            helper(bad, ref, "perturbed")
    R.assert_loss_close(good["loss"][1], ref, "unperturbed", test=True)
    with pytest.raises(AssertionError):
        R.assert_loss_close(good["loss"][1] * (1 + 1e-9), ref, "perturbed", test=True)
    R.assert_scores_close(bd, sref, "unperturbed")
    with pytest.raises(AssertionError):
        R.assert_scores_close(_bump(bd, 7), sref, "perturbed")

    lam, t = 0.05, 1
    case = R.irls_case(family, 30, 1025, "wide", True, True)
    ref, good = R.irls(family, *case, t, 1), R.irls_fp64(family, *case, t, 1, lam)
    i = int(np.argmax(good["wv"]))
    for helper, ok, bad in ((R.assert_wv_close, good["wv"], _bump(good["wv"], i)), (R.assert_z_close, good["z"], _bump(good["z"], i)),
                            (R.assert_ll_close, good["ll"], good["ll"] * (1 + 1e-9))):
        helper(ok, ref, "unperturbed")
        with pytest.raises(AssertionError):
            helper(bad, ref, "perturbed")
    R.assert_gram_close(good["gram"], ref, "unperturbed")
    last = good["gram"].shape[0] - 1
    for entry in ((0, 0), (5, 3), (last, 4), (last, last)):  # intercept, two columns, the z column, z against z
        G = good["gram"].copy()
        G[entry] *= 1.0 + 1e-9
        with pytest.raises(AssertionError):
            R.assert_gram_close(G, ref, "perturbed %s" % (entry,))
    # (the bound of bnext grows with the condition number: 1e-9 in one entry shows where that is small, the mild regime)
    case = R.irls_case(family, 30, 1025, "mild", True, True)
    ref, good = R.irls(family, *case, t, 1), R.irls_fp64(family, *case, t, 1, lam)
    assert R.next_iterate(ref, lam)[1] < 100.0
    R.assert_bnext_close(good["bnext"], ref, lam, "unperturbed")
    with pytest.raises(AssertionError):
        R.assert_bnext_close(_bump(good["bnext"], int(np.argmax(np.abs(good["bnext"])))), ref, lam, "perturbed")


# ---- stand-ins of the defects the GPU file exists to catch -------------------------------------------------------------------
def _slab_shapes():
    for family in (R.LOGISTIC, R.POISSON):
        for nch, T0 in R.SLAB_T0:
            yield family, nch, T0, R.slab_case_n(nch)


def test_a_dropped_row_pair_at_the_end_of_a_short_slab_fails_the_gram_helper():
    """... in the mild regime for both families, for logistic also among the saturated rows (W <= 1 / 4 whatever eta is).
    Beside a Poisson row at e^30 the pair's share of an entry is below the rounding of the entry: no helper can see it
    there, which is why part (b) runs in both regimes."""
    unseen = []
    for family, nch, T0, n in _slab_shapes():
        rows = (nch + 1) * 64
        for regime in R.SLAB_REGIMES:
            case = R.irls_case(family, T0, n, regime, True, True, slab_rows=rows)
            ref = R.irls(family, *case, 1, 1)
            what = "fam%d T0=%d n=%d %s" % (family, T0, n, regime)
            R.assert_gram_close(R.irls_fp64(family, *case, 1, 1)["gram"], ref, what)
            bad = R.irls_fp64(family, *case, 1, 1, drop_rows=[n - 2, n - 1])["gram"]
            if regime == "mild" or family == R.LOGISTIC:
                with pytest.raises(AssertionError):
                    R.assert_gram_close(bad, ref, what + ", last pair dropped")
            else:
                try:
                    R.assert_gram_close(bad, ref, what + ", last pair dropped")
                    unseen.append(what)
                except AssertionError:
                    pass
    # the limitation, pinned: on Poisson's saturating cases the dropped pair goes unseen at some shapes (the helper is not
    # asked to see it there, and the day it sees it everywhere this line says so)
    print("dropped pair unseen at:", unseen)
    assert 1 <= len(unseen) <= len(R.SLAB_T0), unseen


def test_the_working_response_one_gram_column_early_fails_the_gram_helper():
    for family in (R.LOGISTIC, R.POISSON):
        for T0 in R.TEMPLATE_T0:
            mp = (T0 + 2 + 15) // 16 * 16
            for n in (2, 65, 129):
                case = R.irls_case(family, T0, n, "mild", True, True)
                ref = R.irls(family, *case, 0, 1)
                what = "fam%d T0=%d n=%d" % (family, T0, n)
                R.assert_gram_close(R.irls_fp64(family, *case, 0, 1)["gram"], ref, what)
                with pytest.raises(AssertionError):  # at T0 + 2 == 16 mt the slot in front of z is the last active column
                    R.assert_gram_close(R.irls_fp64(family, *case, 0, 1, z_slot=mp - 2)["gram"], ref, what + ", z one slot early")


def test_the_floor_at_t_0_fails_the_row_and_gram_helpers_where_a_weight_is_under_it():
    hit = seen_in_gram = unseen_in_gram = 0
    for name, (family, case, t, wfloor, lam) in R.all_irls_cases().items():
        if t != 0 or not wfloor:
            continue
        ref = R.irls(family, *case, 0, 1)
        live = (ref["wv"] > 0) & (ref["W"].astype(np.float64) < R.FLOOR * (1 - 1e-6))
        bad = R.irls_fp64(family, *case, 0, 1, floor_at_t0=True)
        if live.any():
            hit += 1
            with pytest.raises(AssertionError):
                R.assert_wv_close(bad["wv"], ref, name + ", floor at t = 0")
            if family == R.LOGISTIC or "wide" in name:  # (beside a Poisson row at e^40 a weight of 0.001 is below the rounding)
                seen_in_gram += 1
                with pytest.raises(AssertionError):
                    R.assert_gram_close(bad["gram"], ref, name + ", floor at t = 0")
            else:  # the limitation, pinned below: Poisson, saturating -- at some shapes the Gram helper passes a floor the row helper caught
                try:
                    R.assert_gram_close(bad["gram"], ref, name + ", floor at t = 0 (unseen in the Gram?)")
                    unseen_in_gram += 1
                except AssertionError:
                    pass
        else:  # (nothing under the floor: the defect cannot show, and the helpers must not invent it)
            R.assert_wv_close(bad["wv"], ref, name)
            R.assert_gram_close(bad["gram"], ref, name)
    assert hit >= 8 and seen_in_gram >= 6 and unseen_in_gram >= 1, (hit, seen_in_gram, unseen_in_gram)


def test_the_25_clamp_in_the_training_loss_fails_the_loss_helper():
    hit = 0
    for name, (family, case, lam) in R.all_gh_cases().items():
        if family != R.LOGISTIC:
            continue
        ref = R.gh(family, *case)
        w = np.ones(ref["n"]) if case[2] is None else case[2]
        beyond = (np.abs(ref["eta"].astype(np.float64)) > R.CLAMP_TEST) & (w > 0)
        bad = R.gh_fp64(family, *case, train_clamp=R.CLAMP_TEST)
        if beyond.any():
            hit += 1
            with pytest.raises(AssertionError):
                R.assert_loss_close(bad["loss"][0], ref, name + ", clamp 25")
        else:
            R.assert_loss_close(bad["loss"][0], ref, name)
        R.assert_loss_close(bad["loss"][1], ref, name, test=True)  # (the held-out loss is untouched)
    assert hit >= 6, hit


def test_the_mask_ignored_in_w_fails_the_row_and_gram_helpers():
    hit = 0
    for name, (family, case, t, wfloor, lam) in R.all_irls_cases().items():
        if case[3] is None or "n=16400" in name:
            continue
        ref = R.irls(family, *case, t, wfloor)
        w = np.ones(ref["n"]) if case[2] is None else case[2]
        if not ((case[3] == 0) & (w > 0)).any():
            continue
        hit += 1
        bad = R.irls_fp64(family, *case, t, wfloor, use_mask=False)
        with pytest.raises(AssertionError):
            R.assert_wv_close(bad["wv"], ref, name + ", mask ignored")
        with pytest.raises(AssertionError):
            R.assert_gram_close(bad["gram"], ref, name + ", mask ignored")
    assert hit >= 40, hit
    for name, (family, case, lam) in R.all_gh_cases().items():
        if case[3] is None:
            continue
        ref, bad = R.gh(family, *case), R.gh_fp64(family, *case, use_mask=False)
        w = np.ones(ref["n"]) if case[2] is None else case[2]
        if ((case[3] == 0) & (w > 0)).any():
            with pytest.raises(AssertionError):
                R.assert_h_close(bad["h"], ref, name + ", mask ignored")


# ---- the cases are what they say ---------------------------------------------------------------------------------------------
def test_the_constructed_cases_are_what_their_docstrings_say():
    for mt, nch in R.NCH_OF_MT.items():  # the library's own table (bessx_op_glm_irls_geometry; needs no device)
        assert capi.op_glm_irls_geometry(16 * mt - 2, 100)[1:3] == (mt, nch)
    assert capi.op_glm_irls_geometry(127, 100)[1:3] == (9, 0)
    assert sorted(set((T0 + 2 + 15) // 16 for T0 in R.TEMPLATE_T0)) == list(range(1, 9))
    assert {T0 + 2 for T0 in R.TEMPLATE_T0} >= {16 * mt for mt in range(1, 9)} | {17, 33}
    seen = set()
    for family, T0, n, regime, t, wfloor, weighted, masked in R.template_cases():
        seen |= {("n", n), ("t", t), ("floor", wfloor), ("w", weighted), ("m", masked), ("r", regime), ("mt", (T0 + 2 + 15) // 16, family)}
        assert capi.op_glm_irls_geometry(T0, n)[3] == 64
    assert seen >= {("n", n) for n in R.TEMPLATE_N} | {("t", 0), ("t", 1), ("floor", 0), ("floor", 1), ("w", True), ("w", False),
                                                       ("m", True), ("m", False)} | {("r", r) for r in R.REGIMES}
    assert seen >= {("mt", mt, f) for mt in range(1, 9) for f in (R.LOGISTIC, R.POISSON)}
    assert capi.op_glm_irls_geometry(14, 16400) == (17408, 1, 8, 128)
    # (b): a full group and a one-chunk group in the first slab; the last slab short, with data, its last chunk ragged
    for nch, T0 in R.SLAB_T0:
        rows, n = (nch + 1) * 64, R.slab_case_n(nch)
        ldn = capi.op_glm_irls_geometry(T0, n)[0]
        assert rows // 64 == nch + 1 and n > rows and ldn % rows != 0 and n > ldn - ldn % rows and n % 64 not in (0, 1)
        for regime in R.SLAB_REGIMES:
            case = R.irls_case(R.LOGISTIC, T0, n, regime, True, True, slab_rows=rows)
            assert R.irls(R.LOGISTIC, *case, 1, 1)["wv"][n - 2] > 0  # the last row pair carries weight
        assert {n - 1, 63, rows, rows - 1} <= set(R.special_rows(n, rows))
    assert capi.op_glm_irls_geometry(14, 1100)[0] == 1280 and 1280 % 576 != 0 and 1100 % 64 not in (0, 1)
    for family in (R.LOGISTIC, R.POISSON):
        for regime, lim in R.REGIMES.items():
            X, y, w, mk, cols, b = R.irls_case(family, 30, 1025, regime, True, True)
            assert X.shape == (1025, 33) and len(set(cols.tolist())) == 30 and not np.array_equal(cols, np.sort(cols))
            ref = R.irls(family, X, y, w, mk, cols, b, 1, 1)
            eta = ref["eta"].astype(np.float64)
            rows = R.special_rows(1025) if regime == "saturating" else []
            rest = np.setdiff1d(np.arange(1025), rows)
            assert np.abs(eta[rest]).max() <= lim and (regime == "mild" or np.abs(eta[rest]).max() > 3.0)
            assert (w == 0).any() and w[w > 0].min() >= 0.5 and w.max() <= 2.0
            assert 0.1 < (mk == 0).mean() < 0.3
            if regime == "saturating":
                assert {1024, 63, 64} <= set(rows) and len(rows) == len(R.TARGETS)
                assert np.abs(eta[rows] - np.array(R.TARGETS)).max() < 1e-11
                if family == R.LOGISTIC:
                    assert set(y[rows]) == {0.0, 1.0}
            if family == R.LOGISTIC:
                assert set(y) == {0.0, 1.0}
            else:
                assert y.min() == 0 and y.max() > 50 and (y == np.floor(y)).all()
                if regime != "mild":
                    assert (np.exp(eta) < R.FLOOR).any()
    for family in (R.LOGISTIC, R.POISSON):
        ms, ns, regs = set(), set(), set()
        for name, (fam, case, lam) in R.all_gh_cases().items():
            if fam == family:
                ms.add(len(case[4]))
                ns.add(case[0].shape[0])
                regs.add(name.split()[4])
        assert ms == set(R.GH_M) and ns == set(R.GH_N) and regs == set(R.REGIMES)
    X, y = R.wide_design(R.POISSON)
    assert y.max() > 50 and y.min() == 0
