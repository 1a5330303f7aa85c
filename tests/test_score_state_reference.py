"""CPU: the reference side of tests/test_score_state_gpu.py on exactly its designs and shapes (tests/scorestateref.py).
fp64 NumPy evaluating the library's two score formulas, the residual and the row-block partial sums stays inside the
bounds the GPU file asserts; a score wrong at a relative 1e-9 is far outside them; the exact checks of a state record
reject one swapped pair in A_cur, one stale inA flag, a block extreme from the wrong side and an arg-max that is not the
lowest column of a tie; and the fp64 restatement of the fits says which listed fits end on a repeated active set (the
condition under which the GPU file compares the scores in memory).

fp64 NumPy's own c (printed with -s; 2026-10-21): scores 7.4 (streaming form) and 12.8 (covariance form) on the sweep
designs, 2.7 / 4.7 on the SNR designs; residual 7.5 of u (|y_i| + sum_a |x_ia b_a|) (the 520-column model; 1.9 below 100
columns); row-block partial sums 3.9 of u sum_i |x_ij r_i|; a relative 1e-9 in the largest score needs c >= 4.9e5."""
import numpy as np
import pytest

import scorestateref as R
import xprec

# the sanity figures the GPU file quotes next to its measured constants: fp64 NumPy stays under these
NUMPY_C = {"stream": xprec.SCORE_C_NUMPY, "cov": xprec.SCORE_C_NUMPY, "residual": 16.0, "partials": 16.0}
SEEN = {}
CASES = R.SWEEP + [("snr%g" % lv, R.SNR_SHAPE["n"], R.SNR_SHAPE["p"]) for lv in xprec.SNR_LEVELS] + [R.WIDE, R.CHUNKED]
_CACHE = {}


def _rounded(kind, n, p):
    """The fp64-rounded normalised design (what a library that stores fp64 holds at best), its response and true support."""
    if (kind, n, p) not in _CACHE:
        _CACHE.clear()  # (one design at a time: the cases of a design follow each other)
        X, y, sup, w = R.make_design(kind, n, p)
        Xn, yn = xprec.normalize(X, y, w, 1, True, True)[:2]
        _CACHE[(kind, n, p)] = (Xn.astype(np.float64), yn.astype(np.float64), sup)
    return _CACHE[(kind, n, p)]


def _note(what, v):
    SEEN[what] = max(SEEN.get(what, 0.0), float(v))


def _models(case, Xn, yn, sup, mask, lam):
    """beta = 0, the restricted fit on the true support, and -- for the two wide cases -- the model of their own level."""
    yield sup[:0], np.zeros(0), "beta = 0"
    yield sup, xprec.restricted_fit(Xn, yn, mask, sup, lam)[1]["b64"], "true support"
    if case in (R.WIDE, R.CHUNKED):
        T0 = R.WIDE_T0 if case == R.WIDE else R.CHUNKED_T0
        f = R.pdas_fit(Xn, yn, mask, T0, lam)
        yield f["A"], f["b"], "level %d" % T0


@pytest.mark.parametrize("kind,n,p", CASES)
def test_fp64_numpy_inside_the_bounds_and_1e9_is_caught(kind, n, p):
    assert xprec.EXTENDED
    Xn, yn, sup = _rounded(kind, n, p)
    X_ld = xprec.ld(Xn)
    U, nrb = R.GEOMETRY[n]
    for fold in R.FOLDS:
        mask = R.fold_mask(n, fold)
        if mask is not None:
            assert 0.70 < mask.mean() < 0.80  # 3 of 4 folds
        for lam in R.LAMS:
            for A, b, what in _models((kind, n, p), Xn, yn, sup, mask, lam):
                label = "%s n=%d p=%d fold=%d lam=%g %s" % (kind, n, p, fold, lam, what)
                ref = xprec.scores(Xn, yn, mask, A, b, lam, X_ld)
                for form in ("stream", "cov"):
                    c, j = xprec.score_error_units(xprec.scores_fp64(Xn, yn, mask, A, b, lam, form), ref, form)
                    _note("%s %s" % (form, "snr" if kind.startswith("snr") else "sweep"), c)
                    assert c <= NUMPY_C[form], "%s %s: column %d needs c = %.1f" % (label, form, j, c)
                    # a score vector wrong by a relative 1e-9 in its largest entry is far outside any such c
                    bad = ref["bd"].astype(np.float64)
                    bad[int(np.argmax(bad))] *= 1 + 1e-9
                    cb = xprec.score_error_units(bad, ref, form)[0]
                    _note("1e-9 caught at 1/c", 1.0 / cb)
                    assert cb > 1e4 and cb > 100 * NUMPY_C[form], "%s %s: a 1e-9 error needs only c = %.3g" % (label, form, cb)
                # the residual and the row-block partial sums of the streaming pass, as fp64 NumPy forms them
                r_ref, mag = R.residual(Xn, yn, mask, A, b)
                m = np.ones(n, dtype=bool) if mask is None else mask
                r64 = np.where(m, yn - Xn[:, A] @ b, 0.0)
                c, i = R.residual_error_units(r64, r_ref, mag)
                _note("residual", c)
                assert c <= NUMPY_C["residual"], "%s: residual row %d needs c = %.2f" % (label, i, c)
                rows = 128 * U
                part = np.stack([Xn[rb * rows:(rb + 1) * rows].T @ r64[rb * rows:(rb + 1) * rows] for rb in range(nrb)])
                c, j = R.partial_sum_error_units(part, Xn, r64)
                _note("partials", c)
                assert c <= NUMPY_C["partials"], "%s: partial sums of column %d need c = %.2f" % (label, j, c)
                bad = r64.copy()
                k = int(np.argmax(mag))
                bad[k] += 1e-9 * mag[k]  # (1e-9 of the terms the entry is formed from)
                assert R.residual_error_units(bad, r_ref, mag)[0] > 1e4
                assert R.partial_sum_error_units(part * (1 + 1e-9), Xn, r64)[0] > 10 * NUMPY_C["partials"]
    print("fp64 NumPy so far: " + ", ".join("%s %.3g" % kv for kv in sorted(SEEN.items())))


@pytest.mark.parametrize("kind,n,p", R.SWEEP)
def test_listed_fits_end_on_a_repeated_set(kind, n, p):
    """Every fit of the sweep ends with the set of the iteration before in the fp64 restatement: the GPU file may require
    done && d_fresh of all of them (a fit that ends on a CYCLE leaves scores of the coefficients before its last solve)."""
    Xn, yn, _ = _rounded(kind, n, p)

    def fit(fold, lam, T0, start):
        f = R.pdas_fit(Xn, yn, R.fold_mask(n, fold), T0, lam, *(() if start is None else (start["support"], start["beta"])))
        return {"support": f["A"], "beta": f["b"], "end": f["end"], "iters": f["iters"]}
    count = 0
    for fold, lam, T0, how, f in R.walk_fits(fit):
        count += 1
        assert f["end"] == "repeat", "%s n=%d p=%d fold=%d lam=%g T0=%d %s ends on %s after %d iterations" % (
            kind, n, p, fold, lam, T0, how, f["end"], f["iters"])
    assert count == R.N_FITS


def test_wide_and_limited_fits_end_as_the_gpu_file_expects():
    for (kind, n, p), T0, lams in ((R.WIDE, R.WIDE_T0, R.LAMS), (R.CHUNKED, R.CHUNKED_T0, (R.CHUNKED_LAM,))):
        Xn, yn, _ = _rounded(kind, n, p)
        for lam in lams:
            f = R.pdas_fit(Xn, yn, None, T0, lam)
            assert f["end"] == "repeat", (kind, n, p, T0, lam, f["end"], f["iters"])
    # the two cases built for d_fresh == 0: out of iterations after one solve, and after two without a repeat
    Xn, yn, _ = _rounded(*R.LIMITED)
    for max_iter in (1, 2):
        f = R.pdas_fit(Xn, yn, None, R.LIMITED_T0, 0.0, max_iter=max_iter)
        assert f["end"] == "iterations", (max_iter, f["end"])


def test_the_other_listed_fits_end_on_a_repeated_set():
    """always_select, the tied columns (which must be the largest score outside the set in their block) and the sequences of
    section (e), in the fp64 restatement."""
    X, y, sup, w = R.make_design("iid", 1025, 65)
    always = np.setdiff1d(np.arange(65), sup)[[2, 40]]
    Xn, yn = [a.astype(np.float64) for a in xprec.normalize(X, y, w, 1, True, True)[:2]]
    for fold in R.FOLDS:
        for lam in R.LAMS:
            f = R.pdas_fit(Xn, yn, R.fold_mask(1025, fold), 8, lam, always=always)
            assert f["end"] == "repeat" and set(always) <= set(f["A"]), (fold, lam, f["end"])
    Xt, yt = R.tie_columns(X, y, sup)
    lo, hi = R.tied_pair(sup)
    Xn, yn = [a.astype(np.float64) for a in xprec.normalize(Xt, yt, w, 1, True, True)[:2]]
    assert np.array_equal(Xn[:, lo], Xn[:, hi])
    for lam in R.LAMS:
        f = R.pdas_fit(Xn, yn, None, 8, lam)
        assert f["end"] == "repeat" and lo not in f["A"] and hi not in f["A"]
        mn, mx, arg = R.block_extremes(f["bd"], f["A"], 65)
        assert f["bd"][lo] == f["bd"][hi] == mx[lo // 32] and arg[lo // 32] == lo
    Xn, yn, _ = _rounded(*R.SEQ_CASE)
    fits = []
    for what, T0, lam, fold, start, _ in R.SEQUENCE:
        init = () if start is None else (fits[start]["A"], fits[start]["b"])
        fits.append(R.pdas_fit(Xn, yn, R.fold_mask(R.SEQ_CASE[1], fold), T0, lam, *init))
        assert fits[-1]["end"] == "repeat", (what, fits[-1]["end"], fits[-1]["iters"])


def _state(p=65, T0=8, seed=3):
    """A consistent synthetic state record: a model, its scores (two tied maxima outside the set in block 1) and extremes."""
    rng = np.random.default_rng(seed)
    A = np.sort(rng.choice(p, T0, replace=False)).astype(np.int32)
    b = rng.standard_normal(T0)
    bd = rng.uniform(0.0, 1.0, p)
    bd[A] += 2.0
    out = np.setdiff1d(np.arange(32, 64), A)
    bd[out[3]] = bd[out[7]] = 1.5  # the block's maximum outside the set, twice
    beta = np.zeros(p)
    beta[A] = b
    inA = np.zeros(p, dtype=bool)
    inA[A] = True
    mn, mx, arg = R.block_extremes(bd, A, p)
    assert arg[1] == out[3] and mx[1] == 1.5
    return {"done": 1, "l": 2, "T0": T0, "k_cur": T0, "d_fresh": 1, "has_inA": 1, "A_cur": A, "b_cur": b, "beta_dense": beta,
            "inA": inA, "bd": bd, "bmm_min": mn, "bmm_max": mx, "bmm_arg": arg}, int(out[7])


def test_block_extremes_edge_blocks():
    p = 70
    bd = np.arange(p, dtype=np.float64)
    mn, mx, arg = R.block_extremes(bd, np.arange(32), p)  # block 0 wholly inside, block 1 wholly outside, block 2 short
    assert list(mn) == [0.0, R.DBL_MAX, R.DBL_MAX] and list(mx) == [-1.0, 63.0, 69.0]
    assert list(arg) == [R.NO_COLUMN, 63.0, 69.0]
    bd[40] = R.DBL_MAX  # an always_select column outside the set is the block's maximum
    assert R.block_extremes(bd, np.arange(32), p)[1][1] == R.DBL_MAX and R.block_extremes(bd, np.arange(32), p)[2][1] == 40.0


def test_broken_states_are_rejected():
    st, tied_higher = _state()
    ret = {"support": st["A_cur"].copy(), "beta": st["b_cur"].copy()}
    R.assert_state_consistent(st, ret, "intact")
    R.assert_block_extremes(st, "intact")

    def broken(**kw):
        s = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        s.update(kw)
        return s
    A = st["A_cur"].copy()
    A[[2, 3]] = A[[3, 2]]  # one swapped pair: b_cur no longer belongs to its columns
    with pytest.raises(AssertionError, match="beta_dense"):
        R.assert_state_consistent(broken(A_cur=A), None, "swapped")
    with pytest.raises(AssertionError, match="returned support"):  # ... and swapped consistently, it is not what the call returned
        b = st["b_cur"].copy()
        b[[2, 3]] = b[[3, 2]]
        R.assert_state_consistent(broken(A_cur=A, b_cur=b), ret, "swapped with its coefficients")
    for j in (int(st["A_cur"][0]), int(np.setdiff1d(np.arange(65), st["A_cur"])[0])):  # a stale flag either way
        inA = st["inA"].copy()
        inA[j] = not inA[j]
        with pytest.raises(AssertionError, match="inA"):
            R.assert_state_consistent(broken(inA=inA), None, "stale flag")
    with pytest.raises(AssertionError, match="k_cur"):
        R.assert_state_consistent(broken(T0=9), None, "level")
    mx = st["bmm_max"].copy()
    mx[1] = st["bmm_min"][1]  # an extreme taken from the wrong side
    with pytest.raises(AssertionError, match="maximum outside"):
        R.assert_block_extremes(broken(bmm_max=mx), "wrong side")
    mn = st["bmm_min"].copy()
    mn[0] = st["bmm_max"][0]
    with pytest.raises(AssertionError, match="minimum inside"):
        R.assert_block_extremes(broken(bmm_min=mn), "wrong side")
    arg = st["bmm_arg"].copy()
    arg[1] = tied_higher  # attains the maximum, but is not the lowest column that does
    with pytest.raises(AssertionError, match="column of the maximum"):
        R.assert_block_extremes(broken(bmm_arg=arg), "tie")
    bd = st["bd"].copy()
    bd[int(st["bmm_arg"][2])] *= 1 + 1e-15  # scores re-formed since the extremes were left (one ulp in one entry)
    with pytest.raises(AssertionError):
        R.assert_block_extremes(broken(bd=bd), "stale extremes")
