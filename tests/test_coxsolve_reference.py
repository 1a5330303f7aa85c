"""CPU: the longdouble reference of the Cox solver (tests/coxsolveref.py) against fp64 NumPy on every case of
tests/test_cox_ops_gpu.py.  fp64 NumPy stays inside every bound (this is where SCORE_C is measured); a NumPy stand-in of
the block scan that forms a thread's offset as inclusive - own total fails the risk-set helper on the absorbing cases
and passes on make_cox data; every helper fails on a result that is wrong at 1e-9 in one entry; the constructed cases
are what their docstrings say."""
import numpy as np
import pytest

import coxsolveref as R
import xprec
from bess_amd import synth

pytestmark = pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format here")


def _state_fp64(X, st, w, mk, cols, b):
    """fp64 NumPy stand-in of the state pass.  The risk-set sums are R.scan_standin's additions-only block scan: the
    bound of the sums counts the additions of THAT geometry (scan_depth), which a running sum over n rows exceeds."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    cols = np.asarray(cols, dtype=int)
    w1 = np.ones(n) if w is None else w
    m1 = np.ones(n) if mk is None else mk
    e = np.exp(np.clip(X[:, cols] @ np.asarray(b, dtype=np.float64), -30, 30))
    th = w1 * e * m1
    S0, Sall, Ste = (R.scan_standin(v, "add") for v in (th, e, e * (1 - m1)))
    with np.errstate(divide="ignore"):
        rs0 = np.where(S0 != 0, 1.0 / np.where(S0 != 0, S0, 1.0), 0.0)
    ev = st != 0
    la = (w1[ev] * st[ev] * np.log(e[ev] / Sall[ev])).sum()
    te = ev & (m1 == 0)
    lt = (w1[te] * st[te] * np.log(e[te] / Ste[te])).sum()
    return {"e": e, "theta": th, "s0": S0, "rs0": rs0, "s_all": Sall, "s_test": Ste, "loss": (la, lt)}


def _check_state(got, ref, masked, what):
    R.assert_e_close(got["e"], ref, what)
    R.assert_risk_sums_close(got["s0"], got["theta"], what + " S0", recip=got["rs0"])
    R.assert_risk_sums_close(got["s_all"], got["e"], what + " S_all")
    R.assert_loss_close(got["loss"][0], ref, what)
    if masked:
        R.assert_risk_sums_close(got["s_test"], got["e"] * (1 - ref["mask"]), what + " S_test")
        R.assert_loss_close(got["loss"][1], ref, what + " test rows", test=True)


@pytest.mark.parametrize("n", R.STATE_N)
def test_fp64_numpy_state_stays_inside_every_bound(n):
    for name, (X, st, w, mk, cols, b) in R.state_cases(n).items():
        _check_state(_state_fp64(X, st, w, mk, cols, b), R.state(X, st, w, mk, cols, b), mk is not None,
                     "n=%d %s" % (n, name))


def _all_score_cases():
    for n in R.SCORE_N:
        for p in R.SCORE_P:
            for name, case in R.score_cases(n, p).items():
                yield "n=%d p=%d %s" % (n, p, name), case
    X, st, models = R.absorbing_models()
    for r, (cols, b) in enumerate(models):
        yield "absorbing model %d" % r, (X, st, None, None, cols, b)


def test_fp64_numpy_scores_stay_inside_the_model_and_fix_SCORE_C():
    worst = (0.0, None)
    for what, (X, st, w, mk, cols, b) in _all_score_cases():
        sums = R.score_sums(X, st, w, mk, cols, b)
        for lam in R.SCORE_LAM:
            r, j = R.score_error_units(R.scores_fp64(X, st, w, mk, cols, b, lam), R.scores_finish(sums, lam))
            worst = max(worst, (r, "%s lam=%g column %d" % (what, lam, j)))
    print("fp64 NumPy scores: c = %.4f at %s" % worst)
    assert worst[0] <= R.SCORE_C_NUMPY_MAX * 1.0000001, worst  # the recorded maximum is the measured one
    want = 2.0 ** np.ceil(np.log2(4.0 * R.SCORE_C_NUMPY_MAX))
    assert R.SCORE_C == want, (R.SCORE_C, want)


def test_a_scan_that_subtracts_the_threads_own_total_fails_on_the_absorbing_cases_only():
    X, st, models = R.absorbing_models()
    for r, (cols, b) in enumerate(models):
        e = np.exp(np.clip(X[:, cols[0]] * b[0], -30, 30))
        R.assert_risk_sums_close(R.scan_standin(e, "add"), e, "absorbing %d, additions only" % r)
        with pytest.raises(AssertionError):
            R.assert_risk_sums_close(R.scan_standin(e, "sub"), e, "absorbing %d, inclusive - own" % r)
    Xc, _, stc, sup, beta = synth.make_cox(4100, 40, 4, seed=5)
    e = np.exp(np.clip(Xc[:, sup] @ beta[sup], -30, 30))
    for form in ("add", "sub"):  # (benign data: what the suite had before cannot tell the two forms apart)
        f, _ = R.assert_risk_sums_close(R.scan_standin(e, form), e, "make_cox, " + form)
        assert f < 1.0


def test_the_constructed_cases_are_what_their_docstrings_say():
    X, st, models = R.absorbing_models()
    n = R.ABSORB_N
    assert X.shape == (n, len(R.ABSORB_AT) + 1) and (st == 1).all()
    for r, j0 in enumerate(R.ABSORB_AT):
        scan = X[::-1, r]  # scan index r = row n - 1 - r
        assert (scan[:j0 + 3] == -40.0).all() and scan[j0 + 3] == 40.0 and np.abs(scan[j0 + 4:]).max() < 30.0
        assert (j0 + 3) % R.SC_E == R.SC_E - 1 and j0 % R.SC_E == 0  # the large term is the LAST element of its thread
        ref = R.state(X, st, None, None, *models[r])
        assert float(ref["eta"].max()) == 40.0 and float(ref["e"].max()) == float(np.exp(R.LD(30)))
        S = ref["S_all"][::-1]
        assert float(S[j0 + 2] / S[j0 + 3]) < 2.0 ** -53 / 4  # absorbed: the sums in front vanish beside the term
    assert [(j0 // R.SC_E) % 64 for j0 in R.ABSORB_AT] == [1, 63, 0, 1, 1]
    assert [j0 // R.SC_E // 64 for j0 in R.ABSORB_AT] == [0, 0, 1, 1, 4] and R.ABSORB_AT[-1] // R.SC_B == 1
    stair = X[::-1, -1]
    assert (stair[:7] == -40).all() and (stair[7:11] == 0).all() and stair[11] == 40
    for n in (1, 5, 257):
        cases = R.state_cases(n)
        assert set(len(c[4]) for c in cases.values()) >= {1, 2, 9}
        w = cases["zero weights m=2"][2]
        assert (w == 0).any() and w[n - 1] == 0
        mk = cases["cv mask m=9"][3]
        tail = min(3, n - 1)
        assert (mk[n - tail:] == 0).all() and mk[n - tail - 1] == 1
        if tail:
            assert (R.state(*cases["cv mask m=9"])["S0"][n - tail:] == 0).all()  # empty risk sets
        assert not cases["all censored"][1].any()
        assert np.flatnonzero(cases["last row the only event"][1]).tolist() == [n - 1]
        assert np.flatnonzero(cases["first row the only event"][1]).tolist() == [0]
        if n > 1:
            eta = R.state(*cases["clamp"])["eta"]
            assert float(eta.min()) < -30 and float(eta.max()) > 30


def test_every_helper_fails_on_a_result_that_is_wrong_at_1e_9_in_one_entry():
    n = 1025
    X, st, w, mk, cols, b = R.state_cases(n)["cv mask m=9"]
    ref = R.state(X, st, w, mk, cols, b)
    good = _state_fp64(X, st, w, mk, cols, b)
    _check_state(good, ref, True, "unperturbed")
    i = 300
    assert good["s0"][i] > 0

    def bumped(key):
        a = good[key].copy()
        a[i] *= 1.0 + 1e-9
        return a

    with pytest.raises(AssertionError):
        R.assert_e_close(bumped("e"), ref, "e")
    with pytest.raises(AssertionError):
        R.assert_risk_sums_close(bumped("s0"), good["theta"], "s0")
    with pytest.raises(AssertionError):
        R.assert_risk_sums_close(good["s0"], good["theta"], "rs0", recip=bumped("rs0"))
    empty = good["s0"].copy()
    empty[n - 1] = 1e-300
    with pytest.raises(AssertionError):
        R.assert_risk_sums_close(empty, good["theta"], "empty risk set")
    with pytest.raises(AssertionError):
        R.assert_loss_close(good["loss"][0] * (1.0 + 1e-9), ref, "loss")
    with pytest.raises(AssertionError):
        R.assert_loss_close(good["loss"][1] * (1.0 + 1e-9), ref, "test loss", test=True)
    sref = R.scores(X, st, w, mk, cols, b, 0.05)
    bd = R.scores_fp64(X, st, w, mk, cols, b, 0.05)
    R.assert_scores_close(bd, sref, "unperturbed scores")
    bd[7] *= 1.0 + 1e-9
    with pytest.raises(AssertionError):
        R.assert_scores_close(bd, sref, "scores")


def test_newton_gradient_vanishes_at_the_refined_optimum():
    """newton_gradient_hessian: the gradient against a central difference of the partial likelihood, and Newton steps
    with it reach a point whose gradient is zero to longdouble accuracy."""
    X, _, st, sup, _ = synth.make_cox(600, 40, 4)
    cols = np.sort(sup)
    w = np.random.default_rng(3).uniform(0.5, 2.0, 600)
    b = np.zeros(cols.size, dtype=R.LD)
    for _ in range(12):
        g, H = R.newton_gradient_hessian(X, st, w, None, cols, b, 0.0)
        b = b - R.ld(np.linalg.solve(H.astype(np.float64), g.astype(np.float64)))
    g, H = R.newton_gradient_hessian(X, st, w, None, cols, b, 0.0)
    assert float(np.abs(g).max()) < 1e-15 * float(np.abs(np.diag(H)).max())

    def ll(bb):  # partial log-likelihood as the fit sees it: theta without weights
        eta = R.ld(X[:, cols]) @ bb
        return (R.ld(w * st) * (eta - np.log(R.suffix(np.exp(eta))))).sum()
    b0 = R.ld(np.full(cols.size, 0.1))
    g0, _ = R.newton_gradient_hessian(X, st, w, None, cols, b0, 0.0)
    h = R.LD(1e-6)
    for u in range(cols.size):
        du = np.zeros(cols.size, dtype=R.LD)
        du[u] = h
        fd = (ll(b0 + du) - ll(b0 - du)) / (2 * h)
        assert abs(float(fd - g0[u])) < 1e-8 * max(1.0, abs(float(g0[u])))
