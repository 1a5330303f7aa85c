"""CPU: the extended-precision reference of tests/xprec.py against fp64 NumPy and against the pinned oracle, on the very
inputs tests/test_lm_precision_gpu.py uses.  This is what shows that the REFERENCE ALONE stays inside every bound the GPU
file asserts (a plain fp64 evaluation of each operation uses a small fraction of it; the fraction is in every assertion
message), and that each assertion helper fails on an input that is wrong at the level the suite used to let through."""
import numpy as np
import pytest

import xprec
from oracle import port_ctypes as P

LD = np.longdouble


def _rounded(X, y, w=None, data_type=1):
    """The fp64-rounded normalised design and response (what a library that stores fp64 can hold at best)."""
    w = np.ones(X.shape[0]) if w is None else w
    Xn, yn, xm, xn, ym = xprec.normalize(X, y, w, data_type, True, data_type == 1)
    return Xn.astype(np.float64), yn.astype(np.float64)


@pytest.fixture(scope="module")
def rounded():
    out = {}
    for name in ("iid", "ar1"):
        X, y, sup = xprec.designs()[name]()
        out[name] = _rounded(X, y) + (sup,)
    return out


def test_longdouble_is_the_x86_extended_format():
    assert xprec.EXTENDED and np.finfo(LD).eps < 2e-19 and xprec.U == np.finfo(np.float64).eps / 2


@pytest.mark.parametrize("data_type,is_normal,weighted", [(1, True, True), (1, True, False), (2, True, True),
                                                          (3, True, True), (1, False, True)])
def test_normalize_against_numpy_and_the_oracle(data_type, is_normal, weighted):
    X, y, _ = xprec.design_iid(n=517, p=33, k_true=5)
    X = X * np.linspace(0.5, 3.0, 33) + np.linspace(-2.0, 2.0, 33)
    w = xprec.weights(517) if weighted else np.ones(517)
    add_weight = data_type == 1
    got = xprec.normalize(X, y, w, data_type, is_normal, add_weight)
    want = P.normalize(X, y, w, data_type, is_normal, add_weight)
    for g, o, what in zip(got, want, ("X", "y", "x_mean", "x_norm", "y_mean")):
        if not is_normal and what in ("x_mean", "x_norm", "y_mean"):
            continue
        err = float(np.max(np.abs((xprec.ld(o) - g).astype(np.float64))))
        scale = max(1.0, float(np.max(np.abs(np.asarray(o, dtype=np.float64)))))
        assert err <= 1e-13 * scale, "%s: oracle differs from the longdouble normalisation by %.3e" % (what, err)


def test_normalize_large_means_numpy_stays_inside_the_tolerance():
    """fp64 NumPy as the stand-in for the kernels on the large-mean / wide-scale design: inside
    4 sqrt(n) u (1 + |mean| / sd) on columns and x_norm -- while a flat 1e-13 on x_norm is not met at mean / sd = 1e9."""
    worst_flat = 0.0
    for n, p, f32 in ((130, 33, False), (3001, 1100, False), (1025, 129, True)):
        X, y = xprec.design_large_mean(n, p, fp32_exact=f32)
        if f32:
            assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
        w = xprec.weights(n)
        ref = xprec.normalize(X, y, w, 1, True, True)
        mean = (w @ X) / n
        Xc = X - mean
        norm = np.sqrt(w @ (Xc * Xc))
        Xs = np.sqrt(n) * Xc / norm * np.sqrt(w)[:, None]
        fc, fn = xprec.assert_normalization_close(Xs, mean, norm, ref, w, "fp64 NumPy n=%d p=%d" % (n, p))
        print("normalisation, fp64 NumPy, n=%d p=%d: %.3f of the tolerance on columns, %.3g on x_norm" % (n, p, fc, fn))
        worst_flat = max(worst_flat, float(np.max(np.abs(((norm - ref[3]) / ref[3]).astype(np.float64)))))
        # the helper fails on a column shifted by 100 tolerances
        bad = Xs.copy()
        bad[:, 3] += 100 * xprec.normalization_tolerance(n, ref[2], ref[3])[3] * np.sqrt(w)
        with pytest.raises(AssertionError):
            xprec.assert_normalization_close(bad, mean, norm, ref, w, "shifted")
    assert worst_flat > 1e-13, "a flat 1e-13 on x_norm would do here after all: %.3e" % worst_flat


@pytest.mark.parametrize("name,k,lam", [("iid", 7, 0.0), ("iid", 208, 0.0), ("iid", 254, 0.3), ("iid", 420, 0.0),
                                        ("iid", 1000, 0.0), ("ar1", 65, 0.0), ("ar1", 300, 0.3), ("ar1", 600, 0.0)])
def test_restricted_fit_refinement_and_fp64_solve(rounded, name, k, lam):
    """The refined solution's own KKT residual is at the longdouble level; the plain fp64 solve and the oracle's
    sym_solve sit two orders inside the bound the GPU file asserts, on the designs it uses."""
    Xn, yn, _ = rounded[name]
    A = np.sort(np.random.default_rng(k).choice(Xn.shape[1], k, replace=False))
    mask = xprec.folds(Xn.shape[0]) != 1 if lam else None
    b, info = xprec.restricted_fit(Xn, yn, mask, A, lam)
    assert info["kkt"] < 1e-18, "refined KKT residual %.3e |q|" % info["kkt"]
    f = xprec.assert_fit_close(info["b64"], b, info["cond"], "fp64 solve %s k=%d" % (name, k))
    assert f < 0.01, "fp64 NumPy solve uses %.4f of the bound (cond %.3g)" % (f, info["cond"])
    m = np.ones(Xn.shape[0], bool) if mask is None else mask
    XA = Xn[m][:, A]
    G = XA.T @ XA + lam * np.eye(k)
    f2 = xprec.assert_fit_close(P.sym_solve(G, XA.T @ yn[m]), b, info["cond"], "oracle sym_solve %s k=%d" % (name, k))
    assert f2 < 0.01, "oracle sym_solve uses %.4f of the bound" % f2
    print("%s k=%d lam=%g: cond %.3g, kkt %.2e, fp64 solve %.5f of the bound, oracle %.5f" % (
        name, k, lam, info["cond"], info["kkt"], f, f2))
    # the helper fails on coefficients that are wrong at relative 1e-9
    with pytest.raises(AssertionError):
        xprec.assert_fit_close(b.astype(np.float64) * (1 + 1e-9), b, info["cond"], "perturbed")


def test_reference_reproduces_a_short_oracle_trace():
    """One short path of the pinned oracle: final coefficients of every fit, losses and criteria."""
    X, y, _ = xprec.design_snr(1e-3, n=777, p=60, k_true=6)
    seq = [3, 6, 9]
    t = P.trace(X, y, ic_type=3, sequence=seq)
    Xn, yn = _rounded(X, y)
    assert len(t["fits"]) == len(seq)
    for f, T0, ls, ic in zip(t["fits"], seq, t["loss_calls"], t["ic_calls"]):
        A, b = f["iters"][-1], f["betas"][-1]
        bref, info = xprec.restricted_fit(Xn, yn, None, A, 0.0)
        frac = xprec.assert_fit_close(b, bref, info["cond"], "oracle fit T0=%d" % T0)
        tr, _ = xprec.loss(Xn, yn, None, A, b)
        rel = xprec.assert_loss_close(ls, tr, "oracle loss T0=%d" % T0)
        want_ic = xprec.ic_value(tr, 777, 60, T0, 3)
        assert abs(ic - want_ic) <= 777 * xprec.LOSS_RTOL + 1e-12 * abs(want_ic), (ic, want_ic)
        print("oracle T0=%d: coefficients %.5f of the bound, loss rel %.2e" % (T0, frac, rel))


@pytest.mark.parametrize("level", xprec.SNR_LEVELS)
def test_losses_of_the_snr_designs_in_fp64(level):
    """The designs the suite lacked: tr / yy from 1e-3 down to 1e-13.  The direct sum in fp64 NumPy meets 2e-10 at every
    level (the residual is far above the rounding of y - X b: that line is at tr / yy ~ k u^2 ~ 1e-31)."""
    X, y, sup = xprec.design_snr(level)
    Xn, yn = _rounded(X, y)
    b, info = xprec.restricted_fit(Xn, yn, None, sup, 0.0)
    tr, _ = xprec.loss(Xn, yn, None, sup, b)
    yy = float(yn @ yn) / len(yn)
    assert 0.3 * level < float(tr) / yy < 3 * level, (level, float(tr) / yy)
    b64 = info["b64"]
    e = yn - Xn[:, sup] @ b64
    rel = xprec.assert_loss_close(float(e @ e) / len(yn), xprec.loss(Xn, yn, None, sup, b64)[0], "fp64 direct sum")
    print("tr/yy = %.2e: fp64 direct sum rel %.2e" % (float(tr) / yy, rel))
    with pytest.raises(AssertionError):  # a loss wrong at relative 1e-9 fails
        xprec.assert_loss_close(float(tr) * (1 + 1e-9), tr, "perturbed")
    mask = xprec.folds(len(yn)) != 1
    tr2, te2 = xprec.loss(Xn, yn, mask, sup, b64)
    t = ~mask  # train_loss is over ALL rows whatever the mask, test_loss over the rows outside it, halved
    e64 = yn - Xn[:, sup] @ b64
    assert abs(float(tr2) - float(e64 @ e64) / len(yn)) <= 1e-9 * float(tr2)
    assert abs(float(te2) - float(e64[t] @ e64[t]) / (2 * t.sum())) <= 1e-9 * float(te2)


@pytest.mark.parametrize("name", ["iid", "ar1"] + ["snr%g" % lv for lv in xprec.SNR_LEVELS])
def test_scores_fp64_numpy_inside_the_forward_error_model(name):
    """fp64 NumPy evaluating the SAME two formulas (d from Gram columns; d from the residual) stays inside
    c u S_j pushed through bd = (phi b + d / phi)^2 with c = 64, at beta = 0 and at the fitted model."""
    X, y, sup = xprec.designs()[name]()
    Xn, yn = _rounded(X, y)
    X_ld = xprec.ld(Xn)
    worst = {}
    for lam, mask in ((0.0, None), (0.3, xprec.folds(len(yn)) != 1)):
        b = xprec.restricted_fit(Xn, yn, mask, sup, lam)[1]["b64"]
        for A, bb, what in ((sup[:0], b[:0], "beta = 0"), (sup, b, "fitted")):
            ref = xprec.scores(Xn, yn, mask, A, bb, lam, X_ld)
            for form in ("cov", "stream"):
                r, j = xprec.score_error_units(xprec.scores_fp64(Xn, yn, mask, A, bb, lam, form), ref, form)
                worst[form] = max(worst.get(form, 0.0), r)
                assert r <= xprec.SCORE_C_NUMPY, "%s %s %s: column %d needs c = %.1f" % (name, what, form, j, r)
    print("%s: fp64 NumPy needs c = %.2f (covariance form), %.2f (streaming form)" % (name, worst["cov"], worst["stream"]))
    bad = np.array(ref["bd"], dtype=np.float64)
    j = int(np.argmax(bad))
    bad[j] *= 1 + 1e-9
    assert xprec.score_error_units(bad, ref, "stream")[0] > 1e4  # a score wrong at relative 1e-9 is far outside any c


@pytest.mark.parametrize("n,p", xprec.GRAM_SHAPES)
def test_gram_columns_fp64_numpy_inside_the_bound(n, p):
    X, y = xprec.design_large_mean(n, p)
    w = xprec.weights(n)
    Xn = xprec.normalize(X, y, w, 1, True, True)[0].astype(np.float64)
    cols = (np.arange(min(128, p // 32 * 32)) * 29 + 7) % p
    assert len(set(cols)) == len(cols)
    mask = xprec.folds(n) != 1 if p == 129 else None
    ref = xprec.gram_columns(Xn, mask, cols)
    m = np.ones(n, bool) if mask is None else mask
    got = Xn[m].T @ Xn[m][:, cols]
    norms = np.sqrt((Xn[m] * Xn[m]).sum(axis=0))
    f = xprec.assert_gram_close(got, ref, norms[cols], norms, int(m.sum()), "fp64 NumPy n=%d p=%d" % (n, p))
    assert f < 0.1, "fp64 NumPy uses %.4f of 32 sqrt(n) u |x_j||x_a|" % f
    print("Gram n=%d p=%d: fp64 NumPy uses %.4f of the bound" % (n, p, f))
    bad = got.copy()
    bad[5, 3] += 1e-10 * norms[5] * norms[cols[3]]
    with pytest.raises(AssertionError):
        xprec.assert_gram_close(bad, ref, norms[cols], norms, int(m.sum()), "perturbed")


def test_designs_are_seeded():
    for name, make in xprec.designs().items():
        a, b = make(), make()
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), name
