"""GPU: the LM score values left in device memory against the longdouble reference of tests/xprec.py, read through
Session.score_state (bessx_session_score_state), in both forms of the score pass.  Every comparison is made against
the A_cur, b_cur, lambda and row set the diagnostic itself reports; the reference reads the fp64 columns the library
holds (op_normalize), as in tests/test_lm_precision_gpu.py.  Cases, seeds and helpers: tests/scorestateref.py; the CPU side
(fp64 NumPy inside these bounds, a 1e-9 error outside them, broken states rejected, which fits end on a repeated set):
tests/test_score_state_reference.py.

(a) state consistency, exact, after every fit of every test: beta_dense is b_cur scattered to A_cur, inA its membership,
    k_cur == T0, A_cur / b_cur what the call returned.
(b) streaming sessions: the residual r, the row-block partial sums of k_xtv (added in longdouble, against X^T r of the
    device's own r) and bd, after cold and warm fits at T0 in {1, 8, 33}, lambda in {0, 0.3}, all rows and a fold.
(c) covariance-form sessions WITHOUT tracing, the same fits: bd within SCORE_C, and bitwise the same bd under the hooks
    fuse_sel=0, fuse=0 and chain=0.
(d) cov_bmm == block_extremes(bd, A_cur) exactly whenever bmm_owner names the state's row set; a design with two bitwise
    equal columns outside the support for the lowest-column rule.
(e) sequences that take every branch of enqueue_lm_slot_cov (arg-max start, lambda-only re-score, row-set switch,
    chained paths), the invariant after every fit; (f) reading the state changes neither results nor counters.
A fit that ends with d_fresh == 0 leaves the scores of the iteration before: only the two sessions built for it
(max_iter = 1, 2) may, and there bd is compared with the scores of the model the last iteration started from.

Measured maxima (MI355X, 2026-10-21, on top of commit d8b7e15) and the constants derived from them -- 4 x the maximum,
rounded up to a power of two, the convention SCORE_C was set by; fp64 NumPy's own c for the same check on the same cases
(tests/test_score_state_reference.py) next to it:
  streaming scores, c of the forward-error model      0.878 -> STREAM_SCORE_C = 4  (NumPy 7.4; the cap is xprec.SCORE_C_NUMPY = 64)
  residual r_i / (u (|y_i| + sum_a |x_ia b_a|))       5.93  -> RESID_C = 32        (NumPy 7.53; both at the 520-column model:
                                                                                    k_resid_lm adds 130 products per thread group)
  row-block partial sums / (u sum_i |x_ij r_i|)       1.15  -> PART_C = 8          (NumPy 3.92; U = 1: 1.15, U = 2, 4, 8: 0.63-0.69)
  covariance-form scores of untraced fits             4.06  <= SCORE_C = 8, the project's constant, not redefined here (NumPy
                                                              12.8).  The 1.27 it was derived from came from levels >= 6; the
                                                              largest figures here are level 1 on the AR(1) designs, where
                                                              x_j.y - G_ja b_a cancels most for the neighbours of column a.
Everything in (a), (d), (f) and the hook comparison of (c) is exact equality.
Cost: the file's tests take 5.6 s (11 s with start-up and the references) where tests/test_cov_gpu.py takes 7.8 s in the same
visit; the slowest case 1.6 s (the first session of the process), every other under 1 s.
"""
import numpy as np
import pytest

import scorestateref as R
import xprec
from helpers import hooks
from test_lm_precision_gpu import SCORE_C

pytestmark = pytest.mark.gpu
LD = np.longdouble

# Largest c of every bounded check over all cases of this file, and the constant derived from it: 4 x the maximum, rounded
# up to a power of two (the convention SCORE_C was set by).  "numpy": what fp64 NumPy needs for the same check on the same
# cases (tests/test_score_state_reference.py) -- the sanity figure.
MEASURED = {
    "stream_score": {"max": 0.878, "constant": 4.0, "numpy": 7.4},   # bd of streaming sessions, c of xprec.score_error_units
    "residual": {"max": 5.93, "constant": 32.0, "numpy": 7.53},      # r_i in units of u (|y_i| + sum_a |x_ia b_a|)
    "partials": {"max": 1.15, "constant": 8.0, "numpy": 3.92},       # sum of the row-block partials, units of u sum_i |x_ij r_i|
    "cov_score": {"max": 4.06, "constant": SCORE_C, "numpy": 12.8},  # untraced covariance-form fits: the project's SCORE_C
}
STREAM_SCORE_C = MEASURED["stream_score"]["constant"]
RESID_C = MEASURED["residual"]["constant"]
PART_C = MEASURED["partials"]["constant"]
assert STREAM_SCORE_C <= xprec.SCORE_C_NUMPY
REPORT = {}
K_FOLDS = 4


def _note(what, v):
    REPORT[what] = max(REPORT.get(what, 0.0), float(v))


class _Ref:
    """Designs as the library holds them (op_normalize) and their longdouble copies, by case."""

    def __init__(self, gpu):
        self.gpu, self.data = gpu, {}

    def design(self, kind, n, p, edit=None):
        key = (kind, n, p, edit)
        if key not in self.data:
            X, y, sup, w = R.make_design(kind, n, p)
            if edit == "tied":
                X, y = R.tie_columns(X, y, sup)
            Xs, ys = self.gpu.op_normalize(X, y, w, 1, True, True)[:2]
            Xs = np.ascontiguousarray(Xs)
            self.data[key] = {"X": X, "y": y, "w": w, "sup": sup, "Xs": Xs, "ys": ys, "Xld": xprec.ld(Xs), "n": n, "p": p,
                              "weighted": not kind.startswith("snr")}
        return self.data[key]

    def session(self, d, mode, cv=True, **kw):
        s = self.gpu.Session(d["X"], d["y"], weight=d["w"] if d["weighted"] else None, score_mode=mode, **kw)
        if cv:
            s.set_cv(K_FOLDS, xprec.folds(d["n"]))
        return s


@pytest.fixture(scope="module")
def ref(gpu):
    if not xprec.EXTENDED:
        pytest.skip("np.longdouble is not the x86 extended format on this host: no extended-precision reference")
    yield _Ref(gpu)
    for k in sorted(REPORT):
        print("MEASURED %-40s %.4g" % (k, REPORT[k]))


def _scores_of(d, st, A=None, b=None):
    mask = R.fold_mask(d["n"], st["row_set"] - 1)
    return xprec.scores(d["Xs"], d["ys"], mask, st["A_cur"] if A is None else A, st["b_cur"] if b is None else b,
                        st["lambda"], d["Xld"]), mask


def _expect_fit(st, T0, lam, fold, what, mode):
    """The control block describes the fit just asked for, and that fit ended on a repeated set with fresh sums."""
    assert st["known"] and not st["ahead"], what
    assert (st["T0"], st["lambda"], st["row_set"], st["score_mode"]) == (T0, lam, fold + 1, mode), (what, st["T0"], st["lambda"], st["row_set"])
    assert st["done"] and st["d_fresh"] and not st["info"] and not st["cov_miss"], "%s: done=%d d_fresh=%d info=%d after %d iterations" % (
        what, st["done"], st["d_fresh"], st["info"], st["l"])


def _check_stream(d, st, returned, what, always=()):
    """(a) + (b) for one streaming state."""
    R.assert_state_consistent(st, returned, what)
    assert not st["sums_are_d"] and st["part"].shape == (st["nrb"], d["p"])
    assert (st["U"], st["nrb"]) == R.GEOMETRY[d["n"]], (what, st["U"], st["nrb"])
    sr, mask = _scores_of(d, st)
    r_ref, mag = R.residual(d["Xs"], d["ys"], mask, st["A_cur"], st["b_cur"])
    c, i = R.residual_error_units(st["r"], r_ref, mag)
    print("%s: residual c = %.2f (row %d)" % (what, c, i))
    _note("residual", c)
    assert c <= RESID_C, "%s: residual row %d needs c = %.2f" % (what, i, c)
    c, j = R.partial_sum_error_units(st["part"], d["Xs"], st["r"])
    print("%s: partial sums c = %.2f (column %d)" % (what, c, j))
    _note("partials U=%d" % st["U"], c)
    assert c <= PART_C, "%s: row-block partial sums of column %d need c = %.2f" % (what, j, c)
    c, j = R.score_units(st["bd"], sr, "stream", always)
    print("%s: streaming score c = %.2f (column %d)" % (what, c, j))
    _note("stream_score", c)
    assert c <= STREAM_SCORE_C, "%s: score of column %d needs c = %.2f" % (what, j, c)


def _check_cov(d, st, returned, what, always=(), counts=None):
    """(a), and -- when the block says done && d_fresh for a fit the host has a record of -- (c) and (d)."""
    R.assert_state_consistent(st, returned, what)
    if not (st["done"] and st["d_fresh"] and st["known"]):
        return False
    assert st["sums_are_d"] and st["has_inA"] and not st["info"] and not st["cov_miss"], what
    sr, _ = _scores_of(d, st)
    c, j = R.score_units(st["bd"], sr, "cov", always)
    print("%s: covariance-form score c = %.2f (column %d), bmm_owner %d" % (what, c, j, st["bmm_owner"]))
    _note("cov_score", c)
    assert c <= SCORE_C, "%s: score of column %d needs c = %.2f" % (what, j, c)
    if st["bmm_owner"] == st["row_set"]:
        R.assert_block_extremes(st, what)
        if counts is not None:
            counts["bmm"] = counts.get("bmm", 0) + 1
    if counts is not None:
        counts["scores"] = counts.get("scores", 0) + 1
    return True


def _walk(s, d, mode, check, label):
    """The fit list of tests/scorestateref.py on session s; check(st, returned, what) after every fit.  Returns the states."""
    states = []

    def fit(fold, lam, T0, start):
        if start is None:
            s.reset_caches()
            r = s.fit(T0, lam, fold)
        else:
            r = s.fit(T0, lam, fold, start["support"], start["beta"], start["coef0"])
        st = s.score_state()
        what = "%s fold=%d lam=%g T0=%d %s" % (label, fold, lam, T0, "cold" if start is None else "warm")
        _expect_fit(st, T0, lam, fold, what, mode)
        check(st, r, what)
        states.append(st)
        return r
    n = sum(1 for _ in R.walk_fits(fit))
    assert n == R.N_FITS == len(states)
    return states


# ---- (a) + (b): streaming sessions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,p", R.SWEEP)
def test_streaming_scores_residual_and_partial_sums(gpu, ref, kind, n, p):
    d = ref.design(kind, n, p)
    with ref.session(d, 1) as s:
        _walk(s, d, 1, lambda st, r, what: _check_stream(d, st, r, what), "stream %s n=%d p=%d" % (kind, n, p))
        with pytest.raises(gpu.BessxError) as e:  # no fold contexts on a streaming session
            s.score_state(0)
        assert e.value.code == 1


# ---- (a) + (c) + (d): covariance form, untraced, default launches and under the hooks ------------------------------------------
ROUTES = [None, {"fuse_sel": "0"}, {"fuse": "0"}, {"chain": "0"}]


@pytest.mark.parametrize("kind,n,p", R.SWEEP)
def test_covariance_scores_of_untraced_fits_on_every_route(gpu, ref, monkeypatch, kind, n, p):
    d = ref.design(kind, n, p)
    default = None
    for hk in ROUTES:
        monkeypatch.delenv("BESSX_TEST_HOOKS", raising=False)
        if hk:
            hooks(monkeypatch, **hk)
        label = "cov%s %s n=%d p=%d" % ("" if not hk else " " + ",".join("%s=%s" % kv for kv in hk.items()), kind, n, p)
        counts = {}
        with ref.session(d, 2) as s:
            if hk is None:
                states = _walk(s, d, 2, lambda st, r, what: _check_cov(d, st, r, what, counts=counts), label)
                assert counts["scores"] == R.N_FITS and counts["bmm"] >= R.N_FITS // 2, counts
                default = states
            else:
                def same(st, r, what, k=[0]):
                    R.assert_state_consistent(st, r, what)
                    if st["bmm_owner"] == st["row_set"]:
                        R.assert_block_extremes(st, what)
                    ref_st = default[k[0]]
                    k[0] += 1
                    assert np.array_equal(st["A_cur"], ref_st["A_cur"]) and np.array_equal(st["b_cur"], ref_st["b_cur"]), what + ": model differs from the default route's"
                    assert np.array_equal(st["bd"], ref_st["bd"]), "%s: bd differs from the default route's in %d entries" % (
                        what, int((st["bd"] != ref_st["bd"]).sum()))
                _walk(s, d, 2, same, label)


# ---- the SNR designs, always_select, k_cur > 64, a level above the staging chunk ------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("level", xprec.SNR_LEVELS)
def test_scores_on_the_snr_designs(gpu, ref, level, mode):
    d = ref.design("snr%g" % level, R.SNR_SHAPE["n"], R.SNR_SHAPE["p"])
    k = len(d["sup"])
    with ref.session(d, mode, cv=False) as s:
        cold = s.fit(k, 0.0, -1)
        for r, how in ((cold, "cold"), (None, "warm")):
            if r is None:
                r = s.fit(k, 0.0, -1, cold["support"], cold["beta"], cold["coef0"])
            st = s.score_state()
            what = "snr%g mode %d %s" % (level, mode, how)
            _expect_fit(st, k, 0.0, -1, what, mode)
            if mode == 1:
                _check_stream(d, st, r, what)
            else:
                assert _check_cov(d, st, r, what)


@pytest.mark.parametrize("mode", [1, 2])
def test_always_select_scores_are_dbl_max(gpu, ref, mode):
    d = ref.design("iid", 1025, 65)
    always = tuple(int(j) for j in np.setdiff1d(np.arange(65), d["sup"])[[2, 40]])  # two columns the data would not select
    with ref.session(d, mode, always_select=always) as s:
        for fold in R.FOLDS:
            for lam in R.LAMS:
                s.reset_caches()
                r = s.fit(8, lam, fold)
                assert set(always) <= set(r["support"])
                st = s.score_state()
                what = "always_select mode %d fold=%d lam=%g" % (mode, fold, lam)
                _expect_fit(st, 8, lam, fold, what, mode)
                assert np.all(st["bd"][list(always)] == R.DBL_MAX)
                if mode == 1:
                    _check_stream(d, st, r, what, always)
                else:
                    assert _check_cov(d, st, r, what, always)
                    assert st["bmm_owner"] == st["row_set"] and st["bmm_min"][0] <= R.DBL_MAX


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case,T0,lams", [(R.WIDE, R.WIDE_T0, R.LAMS), (R.CHUNKED, R.CHUNKED_T0, (R.CHUNKED_LAM,))])
def test_scores_of_wide_models(gpu, ref, case, T0, lams, mode):
    """k_cur > 64 (more than one round of the staged coefficients per thread group), and a level above the 512 active
    columns cov_d_body stages per round."""
    d = ref.design(*case)
    with ref.session(d, mode, cv=False) as s:
        for lam in lams:
            s.reset_caches()
            r = s.fit(T0, lam, -1)
            st = s.score_state()
            what = "%s n=%d p=%d mode %d T0=%d lam=%g" % (case + (mode, T0, lam))
            _expect_fit(st, T0, lam, -1, what, mode)
            if mode == 1:
                _check_stream(d, st, r, what)
            else:
                assert _check_cov(d, st, r, what)
                assert st["bmm_owner"] == 0


# ---- (d) ties -----------------------------------------------------------------------------------------------------------------
def test_block_extremes_take_the_lowest_column_of_a_tie(gpu, ref):
    d = ref.design("iid", 1025, 65, "tied")
    lo, hi = R.tied_pair(d["sup"])
    assert np.array_equal(d["Xs"][:, lo], d["Xs"][:, hi]), "the library's copies of the two equal columns differ"
    with ref.session(d, 2, cv=False) as s:
        for lam in R.LAMS:
            s.reset_caches()
            r = s.fit(8, lam, -1)
            st = s.score_state()
            what = "tied columns lam=%g" % lam
            _expect_fit(st, 8, lam, -1, what, 2)
            assert lo not in r["support"] and hi not in r["support"]
            blk = lo // 32
            assert st["bd"][lo] == st["bd"][hi] == st["bmm_max"][blk], "%s: the tie is not the block's maximum outside the set" % what
            assert _check_cov(d, st, r, what) and st["bmm_owner"] == 0
            assert st["bmm_arg"][blk] == lo


# ---- (e) + (f): scores that are kept, not recomputed -----------------------------------------------------------------------------
SEQ_CASE = R.SEQ_CASE
PATH_LEVELS, PATH_LAMS = np.arange(1, 13), (0.0, 0.02, 0.2)


def _sequences(s, look):
    """Every branch of enqueue_lm_slot_cov on one untraced session: look(what, returned) after every fit / path call.
    Returns everything the calls returned."""
    out = []

    def fit(what, T0, lam, fold, start=None):
        r = s.fit(T0, lam, fold) if start is None else s.fit(T0, lam, fold, start["support"], start["beta"], start["coef0"])
        out.append(r)
        look(what, r, T0, lam, fold)
        return r
    s.set_kpath_chains(1)
    fits = []
    for what, T0, lam, fold, start, empty in R.SEQUENCE:
        if empty:
            s.reset_caches()
        fits.append(fit(what, T0, lam, fold, None if start is None else fits[start]))
    # paths: fits chained on the device; whatever fit the control block describes afterwards
    p1 = s.sequential_path(PATH_LEVELS, PATH_LAMS, ic_type=3)
    out.append({k: v for k, v in p1.items() if k not in ("trace", "device_seconds")})
    look("sequential_path", None, None, None, None)
    p2 = s.gs_path(1, 12, ic_type=3)
    out.append({k: v for k, v in p2.items() if k not in ("trace", "device_seconds")})
    look("gs_path", None, None, None, None)
    return out


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


def _counters(s):
    c = s.counters()  # (times, and what the whole process has allocated, are not properties of the sequence)
    return {k: v for k, v in c.items() if not (k.endswith("_ns") or k.endswith("_us") or "process" in k)}


def test_kept_scores_belong_to_the_model_in_memory_and_reading_them_changes_nothing(gpu, ref, monkeypatch):
    monkeypatch.delenv("BESSX_TEST_HOOKS", raising=False)
    d = ref.design(*SEQ_CASE)
    counts, seen = {}, {"not_owner": 0}
    with ref.session(d, 2) as s:
        def look(what, r, T0, lam, fold):
            st = s.score_state()
            if r is not None:
                _expect_fit(st, T0, lam, fold, what, 2)
            held = _check_cov(d, st, r, what, counts=counts)
            if r is not None:
                assert held, what
            else:
                print("%s: the block describes level %d, lambda %g, row set %d (ahead %d): done=%d d_fresh=%d, compared %d" % (
                    what, st["T0"], st["lambda"], st["row_set"], st["ahead"], st["done"], st["d_fresh"], held))
                assert st["known"], what
            seen["not_owner"] += st["bmm_owner"] != st["row_set"]
        watched = _sequences(s, look)
        c_watched = _counters(s)
    with ref.session(d, 2) as s:
        plain = _sequences(s, lambda *a: None)
        c_plain = _counters(s)
    assert _same(watched, plain), "results differ when the state is read after every fit"
    assert c_watched == c_plain, {k: (c_watched[k], c_plain[k]) for k in c_plain if c_watched[k] != c_plain[k]}
    assert c_plain["chained_fits"] > 0, c_plain  # (the paths did chain on the device: reading the state broke no chain)
    assert counts["scores"] >= 16 and counts["bmm"] >= 12, counts


@pytest.mark.parametrize("max_iter", [1, 2])
def test_fits_that_end_without_fresh_scores(gpu, ref, monkeypatch, max_iter):
    """Out of iterations: d_fresh == 0, bd is the score vector of the model the LAST iteration started from -- which is
    compared -- and nothing of it is kept for the fit that follows: that fit returns, bit for bit, what a fresh session
    returns from the same start, and once a fit ends on a repeated set the invariant holds again."""
    monkeypatch.delenv("BESSX_TEST_HOOKS", raising=False)
    d = ref.design(*R.LIMITED)
    T0 = R.LIMITED_T0
    with ref.session(d, 2, cv=False, max_iter=max_iter) as s:
        start, recovered = None, False
        for k in range(8):
            r = s.fit(T0, 0.0, -1) if start is None else s.fit(T0, 0.0, -1, start["support"], start["beta"], start["coef0"])
            st = s.score_state()
            what = "max_iter=%d fit %d" % (max_iter, k)
            R.assert_state_consistent(st, None, what)
            assert st["known"] and st["T0"] == T0 and st["l"] <= max_iter
            with ref.session(d, 2, cv=False, max_iter=max_iter) as fresh:
                want = fresh.fit(T0, 0.0, -1) if start is None else fresh.fit(T0, 0.0, -1, start["support"], start["beta"], start["coef0"])
            assert _same(r, want), what + ": differs from a fresh session started from the same model"
            if st["done"] and st["d_fresh"]:
                assert max_iter == 2 and k > 0, what
                assert _check_cov(d, st, r, what)
                recovered = True
                break
            assert k > 0 or st["d_fresh"] == 0
            if max_iter == 1:
                # one iteration: the scores in memory are those of the model the fit started from
                A = np.zeros(0, dtype=int) if start is None else start["support"]
                b = np.zeros(0) if start is None else start["beta"]
                sr, _ = _scores_of(d, st, A, b)
                c, j = R.score_units(st["bd"], sr, "cov")
                _note("cov_score", c)
                assert c <= SCORE_C, "%s: score of column %d needs c = %.2f against the model the iteration started from" % (what, j, c)
            start = r
        assert recovered == (max_iter == 2)


# ---- fold contexts ----------------------------------------------------------------------------------------------------------------
def test_fold_contexts_and_refusals(gpu, ref, monkeypatch):
    monkeypatch.delenv("BESSX_TEST_HOOKS", raising=False)
    d = ref.design(*SEQ_CASE)
    with ref.session(d, 2, cv=False) as s:
        with pytest.raises(gpu.BessxError) as e:  # no folds, no contexts
            s.score_state(0)
        assert e.value.code == 1
    with ref.session(d, 2) as s:
        before = None
        for T0 in (8, 9):
            recs = s.cv_eval(T0, 0.3, True, folds=list(range(K_FOLDS)), **({} if before is None else {
                "init_idx": before["support"], "init_val": before["beta"]}))
            before = recs[0]
            if s.counters()["cv_fold_contexts"] == 0:
                pytest.fail("the side-by-side fold chains were not set up on this session")
            for k in range(K_FOLDS):
                st = s.score_state(k)
                what = "fold context %d T0=%d" % (k, T0)
                assert (st["row_set"], st["lambda"], st["T0"]) == (k + 1, 0.3, T0), what
                assert st["done"] and st["d_fresh"], what
                assert _check_cov(d, st, recs[1 + k], what)
        with pytest.raises(gpu.BessxError):
            s.score_state(K_FOLDS)
    X, y, _, _ = R.make_design("iid", 130, 33)
    with gpu.Session(X, (y > np.median(y)).astype(float), model_type=2, data_type=2) as s:  # logistic: pinned by its own files
        with pytest.raises(gpu.BessxError) as e:
            s.score_state()
        assert e.value.code == 3
    with gpu.Session(X, y, g_index=np.arange(0, 33, 3)) as s:  # groups of three columns
        with pytest.raises(gpu.BessxError) as e:
            s.score_state()
        assert e.value.code == 3
