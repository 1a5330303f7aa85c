"""GPU: the Cox solver's state pass, risk-set scans, loss sums and sacrifice scores, each called alone through the C ABI
(bessx_op_cox_state / _score / _score_multi), against the longdouble reference of tests/coxsolveref.py.  The bounds live
in coxsolveref.assert_*; tests/test_coxsolve_reference.py shows on the CPU that fp64 NumPy sits inside them, that every
helper fails on a result wrong at 1e-9, and that a block scan which forms a thread's offset as inclusive - own total
fails the risk-set helper on the absorbing cases of (b) while passing on make_cox data.

(a) state and scans over the row counts at which the scan's geometry changes, (b) the absorbing pattern at lane, wave
and block boundaries, (c) scores in both forms and the multi-chain pass, (d) run to run, (e) the loss a session's fit
returns.

Not covered here.  k_cox_hess (both forms), k_cox_M_*, k_cox_nvec*, k_cox_car, k_cox_cscan_* and the line search
k_cox_ls5_* have no op-level entry: the Newton step is reached only through Session.fit, whose coefficients are those of
a cold-started Newton iteration stopped by the reference's rule |ll0 - ll1| < 1e-5 |0.1 + ll0| (it returns the iterate
BEFORE the last step), so their distance from the optimum is set by that rule and not by rounding.  A fixed-point test
(warm start at the longdouble optimum, coefficients back within 16 one-step rounding shifts) is therefore NOT here:
Algorithm::fit refits from zero whatever the warm start is.  (e) checks what does not depend on the number of steps: the
returned loss IS the loss of the returned coefficients.  The group branch of get_A (need_uv) is not reached either.

Measured maxima per bound and the file's wall time next to tests/test_cox_gpu.py's: NOT recorded yet -- this file has not
run on an MI355X (every test prints the fraction of each bound it uses, -s shows them).  The bounds do not depend on
them: SCORE_C comes from fp64 NumPy on the CPU (coxsolveref.SCORE_C_NUMPY_MAX), the rest is derived."""
import numpy as np
import pytest

import coxsolveref as R
import xprec

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format")]


def _state(gpu, X, st, w, mk, cols, b):
    return gpu.op_cox_state(X, st, cols, b, weight=w, mask=mk)


def _check_state(got, ref, masked, what):
    f = {"e": R.assert_e_close(got["e"], ref, what)}
    f["s0"], f["rs0"] = R.assert_risk_sums_close(got["s0"], got["theta"], what + " S0", recip=got["rs0"])
    f["s_all"], _ = R.assert_risk_sums_close(got["s_all"], got["e"], what + " S_all")
    f["loss"] = R.assert_loss_close(got["loss"][0], ref, what)
    # theta is w e mask formed from the returned e: two products
    want = (R.ld(got["e"]) * (ref["theta"] / ref["e"])).astype(np.float64)
    assert np.all(np.abs(got["theta"] - want) <= 2 * R.U * np.abs(want)), what + " theta"
    if masked:
        f["s_test"], _ = R.assert_risk_sums_close(got["s_test"], got["e"] * (1 - ref["mask"]), what + " S_test")
        f["loss_test"] = R.assert_loss_close(got["loss"][1], ref, what + " test rows", test=True)
    else:
        assert got["s_test"] is None and got["loss"][1] == 0.0
    return f


def _same(a, b):
    for k in a:
        if a[k] is None:
            assert b[k] is None
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


# ---- (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.STATE_N)
def test_state_pass_and_scans(gpu, n):
    for name, case in R.state_cases(n).items():
        X, st, w, mk, cols, b = case
        got = _state(gpu, *case)
        _check_state(got, R.state(*case), mk is not None, "n=%d %s" % (n, name))
        _same(got, _state(gpu, *case))  # (d)
        if not st.any():
            assert got["loss"][0] == 0.0 and got["loss"][1] == 0.0


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def test_small_risk_sets_behind_a_large_term_of_the_same_thread(gpu):
    """Sums, reciprocals, loss and scores on coxsolveref.absorbing_models(): S at the three rows in front of the e^30 term
    of their own thread is a handful of e^-30 and has to come out to full relative accuracy."""
    X, st, models = R.absorbing_models()
    for r, (cols, b) in enumerate(models):
        what = "absorbing model %d" % r
        got = _state(gpu, X, st, None, None, cols, b)
        ref = R.state(X, st, None, None, cols, b)
        _check_state(got, ref, False, what)
        _same(got, _state(gpu, X, st, None, None, cols, b))
        sums = R.score_sums(X, st, None, None, cols, b)
        for lam in R.SCORE_LAM:
            sref = R.scores_finish(sums, lam)
            bd = [gpu.op_cox_score(X, st, cols, b, lam=lam, form=form) for form in (0, 1)]
            for form in (0, 1):
                R.assert_scores_close(bd[form], sref, "%s lam=%g form %d" % (what, lam, form))
            # (the columns coxsolveref.score_ill_conditioned names are left out by the helper)
            R.assert_scores_close(bd[0], dict(sref, bd=R.ld(bd[1])), what + " form 0 against form 1", c=2 * R.SCORE_C)


# ---- (c) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SCORE_N)
def test_scores_in_both_forms(gpu, n):
    """bd of both forms within SCORE_C of the forward-error model, and within twice that of each other; every call twice,
    bitwise the same."""
    worst = 0.0
    for p in R.SCORE_P:
        for name, (X, st, w, mk, cols, b) in R.score_cases(n, p).items():
            sums = R.score_sums(X, st, w, mk, cols, b)
            for lam in R.SCORE_LAM:
                sref = R.scores_finish(sums, lam)
                assert not R.score_ill_conditioned(sref).any()
                what = "n=%d p=%d %s lam=%g" % (n, p, name, lam)
                bd = [gpu.op_cox_score(X, st, cols, b, lam=lam, form=form, weight=w, mask=mk) for form in (0, 1)]
                for form in (0, 1):
                    worst = max(worst, R.assert_scores_close(bd[form], sref, what + " form %d" % form))
                    assert np.array_equal(bd[form], gpu.op_cox_score(X, st, cols, b, lam=lam, form=form, weight=w, mask=mk))
                R.assert_scores_close(bd[0], dict(sref, bd=R.ld(bd[1])), what + " form 0 against form 1", c=2 * R.SCORE_C)
    print("n=%d: largest c of the scores %.3f" % (n, worst))


@pytest.mark.parametrize("nc", [1, 2, 5, R.COX_MC_MAX])
def test_multi_chain_score_pass_is_bitwise_the_single_pass(gpu, nc):
    """k_cox_score1p_mc walks, per chain, the rows of a row block bottom-up with the same fused multiply-adds and leaves
    the same five sums per (row block, column) and P0 per row block as k_cox_score1p (its sub-tiles are 16 rows instead of
    32, which does not change the order of a column's walk), and k_cox_score_1p folds them: the same sums in the same
    order, so the scores are bitwise those of nc single passes."""
    for n, p in ((97, 9), (1025, 33), (4100, 257)):
        X, st, w, mk = R.score_data(n, p)
        cols = R.score_models(p)["three"][0]
        bs = np.random.default_rng(nc).uniform(-0.8, 0.8, (nc, cols.size))
        bs[0] = 0.0
        for ww, mm in ((None, None), (w, mk)):
            got = gpu.op_cox_score_multi(X, st, cols, bs, lam=0.05, weight=ww, mask=mm)
            assert got.shape == (nc, p)
            for c in range(nc):
                assert np.array_equal(got[c], gpu.op_cox_score(X, st, cols, bs[c], lam=0.05, form=1, weight=ww, mask=mm))
            assert np.array_equal(got, gpu.op_cox_score_multi(X, st, cols, bs, lam=0.05, weight=ww, mask=mm))


# ---- (e) ---------------------------------------------------------------------------------------------------------------
def _fit_and_check_loss(gpu, X, st, T0, what):
    with gpu.Session(X, st, data_type=3, model_type=4, is_normal=False) as s:
        got = s.fit(T0)
    ref = R.state(X, st, None, None, got["support"], got["beta"])
    # train_loss = -2 sum_i w_i delta_i log(e_i / S_i): the bound of the sum, doubled (the product with -2 is exact)
    err, bound = float(abs(R.LD(got["train_loss"]) + 2 * ref["loss_all"])), 2 * R.loss_bound(ref)
    print("%s: train_loss %.17g, |error| %.3e = %.3f of the bound; eta in [%.2f, %.2f]" % (
        what, got["train_loss"], err, err / bound, float(ref["eta"].min()), float(ref["eta"].max())))
    assert np.isfinite(got["train_loss"]) and err <= bound, (what, got["train_loss"], float(-2 * ref["loss_all"]), err, bound)
    return ref


def test_the_loss_a_fit_returns_is_the_loss_of_its_coefficients(gpu):
    from bess_amd import synth
    X, _, st, _, _ = synth.make_cox(600, 40, 4)
    _fit_and_check_loss(gpu, X, st, 4, "make_cox(600, 40, 4)")
    X, st = R.outlier_design()
    ref = _fit_and_check_loss(gpu, X, st, 3, "outlier design")
    assert float(ref["eta"].min()) < -12.0 and float(ref["eta"].max()) > 12.0, "the outlier design no longer spans +-12"
