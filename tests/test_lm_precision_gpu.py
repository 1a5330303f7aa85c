"""GPU: LM fits, losses, scores, Gram columns and the normalisation against the extended-precision reference of
tests/xprec.py (np.longdouble), through the existing C ABI (capi.Session, op_normalize).  The bounds are the issue's and
live in xprec.assert_*; tests/test_xprec_reference.py shows on the CPU that fp64 NumPy and the oracle sit far inside them
and that every helper fails on a result that is wrong at 1e-9.

Which design the reference reads.  (e) compares the library's normalisation with xprec.normalize on the LONGDOUBLE
design (the question is the normalisation).  (a)-(d) ask about the solvers, the loss sums, k_cov_d and the panel kernels,
so their reference reads the fp64 columns the library itself holds: the output of op_normalize, the kernel the session
runs (k_col_normalize: one workgroup per column, independent of the row padding; (e) checks that a session's x_mean /
x_norm are bitwise op_normalize's).

Covered elsewhere: the score VALUES beyond what (c) sees here.  cov_state serves the covariance form only, and (c) reads it
after TRACED fits (the trace names the model the last scores were formed from); tracing switches the fused selection +
solve launch (k_sel_cgr), the chained start, the lambda-only re-score and the arg-max start off.  tests/test_score_state_gpu.py
reads the whole score state through bessx_session_score_state -- control block, A_cur / b_cur, bd, the sums bd was formed
from, the per-block extremes of k_cov_d -- and holds to xprec.scores: the scores of STREAMING sessions after fits (with the
residual and k_xtv's row-block partial sums, at every U and at nrb % 4 != 0), the scores of UNTRACED covariance-form fits on
the default launches and bitwise under fuse_sel=0 / fuse=0 / chain=0, and the scores that are kept instead of recomputed
(chained paths, row-set switches).  Gram columns of a CV row set are not compared HERE (the
prefill export serves row set 0 of sessions without folds only): tests/test_cv_gram_gpu.py holds every row set's cached
columns -- shared fills, masked fills, the refused fold-major copy, more than one slab per fold -- to the same bound through
bessx_session_cov_cache_columns.  The hand-over at CGB_MAX_K from bessx_cgbig.hip to the blocked Cholesky is listed in
LARGE_T0 and runs in its own test.
Here the fused launches are held to the coefficient and loss bounds of (a); their score values are in that file too.
marginal_scores is host arithmetic on x_j.y and x_j.x_j read back from the device: it covers the kernels that form those
sums, not k_score / k_cov_d.

Measured maxima (MI355X, 2026-10-16, on top of commit 9b20946):
  restricted fits, |b - b*| / bound, all routes                      0.011   (collinear, lam = 0.3; benign designs 0.0025;
                                                                              T0 = 4096 / 4097 at lam = 2 n: 0.0006 / 0.005)
  train_loss, relative, sweep + SNR designs (bound 2e-10)            4.1e-11 (tr/yy = 1e-13, covariance form, path: 2.4e-11;
                                                                              at the 1e-6 guard: 6.4e-15); test_loss 7.6e-15
  scores, c of the forward-error model                               1.27 (marginal), 0.56 (after a fit) -> SCORE_C = 8
  Gram entries / (32 sqrt(n) u |x_j||x_a|)                           0.023
  normalisation, columns / tolerance, x_norm / tolerance             0.047, 3.6e-5
  The score gap at the selection boundary exceeded the error bound in all 16 fits of (c): the selection is asserted there.
Cost: the file takes 47.6 s where tests/test_cov_gpu.py takes 7.0 s in the same visit -- 6.8 times, NOT under the factor two
that was asked.  18 s are the two fits at CGB_MAX_K / CGB_MAX_K + 1 (12301 x 5296 design, and their longdouble
reference: a 4096 x 4096 Gram, its eigenvalues and four refinement rounds on the CPU); each streaming sweep takes ~3 s
(k_gram + k_chol_big at every level, five sessions: 14 s), the covariance sweeps 0.4-0.8 s each (eleven: 7 s), Gram /
normalisation / scores / SNR designs the rest.  One session per design / mode / hook set and one reference per distinct
support are in place; what remains is the list of cases itself (25 levels x 2 lambda x cold / warm x 16 sessions).
Which solver answered (cg_fallbacks per fit, printed by the sweep).  Register-resident solvers: 0 fallbacks wherever 64
steps must suffice (iid, and ar03 = AR(1) with rho = 0.3, every level up to T0_FAST + 1).  bessx_cgbig.hip: the iid
sweep's 8 fallbacks are the cold fits at T0 = 300 (lam = 0.3), 420, 600 and 1000, one each -- the solve that finds the
step guess left by the previous, warm fit too short; at most 1 per fit is asserted where 64 steps must suffice, and 0 in
fresh sessions (40 queued steps) at T0 = 256, 420, 600 and CGB_MAX_K with a ridge that makes 40 provably enough.  On
the ar1 design (rho = 0.9) the conjugate gradients hand most systems to the fallback (585 per sweep): nothing is
required there, both solvers are held to the same bound.  "Cholesky answered" is asserted on the collinear path 1..24
(14 fallbacks), on which tests/test_cov_gpu.py requires it already; single fits at 8, 12, 24 columns of that design are
solved by the conjugate gradients (0 fallbacks).
"""
import os
import re

import numpy as np
import pytest

import xprec
from helpers import hooks

pytestmark = pytest.mark.gpu
LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bess_amd", "csrc")

# largest c = |bd - bd*| / (forward-error model with c = 1) observed over all cases of (c), see test_scores_*:
# raw maximum and the constant derived from it (x 4, rounded up to a power of two)
MEASURED = {"score_ratio_max": 1.266, "SCORE_C": 8.0}
SCORE_C = MEASURED["SCORE_C"]


def _constant(fname, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, fname)).read())
    assert m, "%s no longer states %s: re-derive the dispatch boundaries of this test" % (fname, pattern)
    return int(m.group(1))


CGB_MAX_K = _constant("bessx_dev.h", r"constexpr int CGB_MAX_K = (\d+);")
T0_FAST = _constant("bessx_host.h", r"static constexpr int T0_FAST = (\d+);")
CGR_ROWS = _constant("bessx_k_solve.hip", r"bool sel_cgr_applies\(int len, int m\) \{ return .* m <= (\d+); \}")
# waves own k/8 columns (7, 8, 9), tiles of 16 and 64, the row-dealt solver's limit, the register-resident solvers' limit
# (T0_FAST with an intercept, T0_FAST + 1 without), the first systems of bessx_cgbig.hip / k_chol_big, larger ones
T0_SWEEP = sorted({1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, CGR_ROWS - 1, CGR_ROWS, CGR_ROWS + 1, T0_FAST,
                   T0_FAST + 1, T0_FAST + 2, T0_FAST + 3, 300, 420, 600, 1000})
LARGE_T0 = (CGB_MAX_K, CGB_MAX_K + 1)
LAMS = (0.0, 0.3)
ROUTES = {"streaming": (1, {}), "cov": (2, {}), "cov-tiles": (2, {"cg_layout": "tiles"}),
          "cov-chol": (2, {"cov_solver": "chol"}), "cov-fuse_sel0": (2, {"fuse_sel": "0"}), "cov-fuse0": (2, {"fuse": "0"})}
REPORT = {}  # what -> largest figure seen; printed when the module's fixture is torn down
CG_REQUIRED = {}  # (sweep label, bessx_cgbig.hip?) -> fits on which the conjugate gradients were required to answer
CGB_GUESS_FIRST = _constant("bessx_host.h", r"cgb_guess = (\d+);")
CGB_GUESS_MIN = _constant("bessx_fit.cpp", r"s->cgb_guess = std::max\((\d+), std::min\(64, hc->irls_last \+ 8\)\);")


def _note(what, value):
    REPORT[what] = max(REPORT.get(what, 0.0), float(value))


@pytest.fixture(scope="module")
def ref(gpu):
    if not xprec.EXTENDED:
        pytest.skip("np.longdouble is not the x86 extended format on this host: no extended-precision reference")
    yield _Ref(gpu)
    for k in sorted(REPORT):  # the largest figures of this run (the source of the table in the header; shown with -s)
        print("MEASURED %-60s %.4g" % (k, REPORT[k]))


class _Ref:
    """The designs as the library holds them, their longdouble copies, and the reference fits by support."""

    def __init__(self, gpu):
        self.gpu, self.data, self.fits = gpu, {}, {}

    def design(self, name, weighted=False):
        key = (name, weighted)
        if key not in self.data:
            X, y, sup = xprec.designs()[name]()
            w = xprec.weights(len(y)) if weighted else np.ones(len(y))
            Xs, ys = self.gpu.op_normalize(X, y, w, 1, True, True)[:2]
            self.data[key] = {"X": X, "y": y, "w": w, "sup": sup, "Xs": np.ascontiguousarray(Xs), "ys": ys,
                              "Xld": xprec.ld(Xs)}
        return self.data[key]

    def fit(self, name, weighted, mask_key, mask, lam, support):
        key = (name, weighted, mask_key, lam, np.asarray(support, dtype=np.int32).tobytes())
        if key not in self.fits:
            d = self.design(name, weighted)
            b, info = xprec.restricted_fit(d["Xs"], d["ys"], mask, support, lam)
            # the reference's own residual: 100 x under the 1e-13 it has to resolve (1e-19 on benign supports; up to 5e-17 at
            # cond 1e9 on the collinear design, where longdouble rounding times |G||b| / |q| is what remains)
            assert info["kkt"] < 1e-15, "reference refinement did not converge: %.3e" % info["kkt"]
            self.fits[key] = (b, info["cond"])
        return self.fits[key]


def _check_fit(ref, name, weighted, mask_key, mask, lam, T0, r, what):
    """One fit record against the reference on ITS support: coefficients, train_loss, test_loss.  Returns 1."""
    d = ref.design(name, weighted)
    sup = r["support"]
    assert len(sup) == T0 and len(np.unique(sup)) == T0 and len(r["beta"]) == T0, "%s: support of the wrong length" % what
    b_ref, condG = ref.fit(name, weighted, mask_key, mask, lam, sup)
    _note("fit/bound " + what.split(" T0=")[0], xprec.assert_fit_close(r["beta"], b_ref, condG, what))
    e = d["ys"].astype(LD) - d["Xld"][:, sup] @ xprec.ld(r["beta"])
    tr = (e @ e) / LD(e.size)
    _note("loss rel " + what.split(" T0=")[0], xprec.assert_loss_close(r["train_loss"], tr, what + " train_loss"))
    if mask is not None:
        t = ~mask
        te = (e[t] @ e[t]) / LD(2 * int(t.sum()))
        _note("test loss rel " + what.split(" T0=")[0], xprec.assert_loss_close(r["test_loss"], te, what + " test_loss"))
    return 1


COND_SLACK = 2.0  # the systems of a fit's earlier iterations differ from the final support in a few columns


def _cg_steps(condG):
    """Steps after which conjugate gradients MUST have reached the 1e-13 residual on a system of this condition number:
    the smallest N with 2 sqrt(cond) ((sqrt(cond) - 1) / (sqrt(cond) + 1))^N <= 1e-14 (the textbook bound on the energy-norm
    error, sqrt(cond) to turn it into a residual, ten times below the target)."""
    rc = np.sqrt(max(condG, 1.0 + 1e-12))
    return int(np.ceil(np.log(1e-14 / (2 * rc)) / np.log((rc - 1) / (rc + 1))))


def _is_cgbig(T0):
    return T0_FAST + 1 < T0 <= CGB_MAX_K


def _allowed_fallbacks(condG, T0):
    """How many Cholesky fallbacks ONE fit may count, from the condition number of its final system (times COND_SLACK), or
    None where nothing can be required.  Register-resident solvers (T0 <= T0_FAST + 1): up to 64 steps in one launch --
    0 if 64 steps must suffice.  bessx_cgbig.hip (up to CGB_MAX_K): one launch per step, as many as the session's guess
    says (CGB_GUESS_FIRST in a fresh session, then the last solve's steps + 8, never under CGB_GUESS_MIN; 64 for the rest
    of a fit after a fallback): 0 if CGB_GUESS_MIN steps must suffice, at most 1 -- the solve that found the guess short --
    if 64 must.  test_large_conjugate_gradients_answer_in_a_fresh_session shows them answering with a known guess."""
    N = _cg_steps(COND_SLACK * condG)
    if T0 <= T0_FAST + 1:
        return 0 if N <= 64 else None
    if _is_cgbig(T0):
        return 0 if N <= CGB_GUESS_MIN else (1 if N <= 64 else None)
    return None


def _sweep(ref, s, name, weighted, fold, label, t0s=T0_SWEEP, must_cg=False):
    """Every T0 x lambda, cold and warm from the previous level's model.  Returns the number of checks made."""
    mask = None if fold < 0 else xprec.folds(s.n) != fold
    done = 0
    for lam in LAMS:
        prev = None
        for T0 in t0s:
            what = "%s lam=%g T0=%d" % (label, lam, T0)
            s.reset_caches()
            c0 = s.counters()["cg_fallbacks"]
            cold = s.fit(T0, lam, fold)
            c1 = s.counters()["cg_fallbacks"]
            done += _check_fit(ref, name, weighted, fold, mask, lam, T0, cold, what + " cold")
            prev = cold if prev is None else prev
            warm = s.fit(T0, lam, fold, prev["support"], prev["beta"], prev["coef0"])
            c2 = s.counters()["cg_fallbacks"]
            done += _check_fit(ref, name, weighted, fold, mask, lam, T0, warm, what + " warm")
            prev = cold
            # which solver answered, fit by fit (every system of a PDAS iteration counts)
            for r, fell, kind in ((cold, c1 - c0, "cold"), (warm, c2 - c1, "warm")):
                condG = ref.fit(name, weighted, fold, mask, lam, r["support"])[1]
                allowed = _allowed_fallbacks(condG, T0) if must_cg else None
                if fell:
                    print("%s %s: %d Cholesky fallback(s), cond %.3g, allowed %s" % (what, kind, fell, condG, allowed))
                if allowed is not None:
                    CG_REQUIRED[(label, T0 > T0_FAST + 1)] = CG_REQUIRED.get((label, T0 > T0_FAST + 1), 0) + 1
                    assert fell <= allowed, "%s %s: %d system(s) handed to Cholesky, cond %.3g needs %d CG steps at most" % (
                        what, kind, fell, condG, _cg_steps(COND_SLACK * condG))
    return done


# ---- (a) + (b, first half): every solver route -------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", [(n, r) for n in ("iid", "ar1") for r in ROUTES] + [("ar03", "cov")])
def test_restricted_fits_and_losses_on_every_route(gpu, ref, monkeypatch, name, route):
    mode, hk = ROUTES[route]
    if hk:
        hooks(monkeypatch, **hk)
    d = ref.design(name)
    with gpu.Session(d["X"], d["y"], score_mode=mode) as s:
        assert s.score_mode() == mode
        cg = mode == 2 and hk.get("cov_solver") != "chol"
        label = "%s %s" % (name, route)
        done = _sweep(ref, s, name, False, -1, label, must_cg=cg)
        if cg and name in ("iid", "ar03"):
            # the assertion is not vacuous: on the iid design and on the mildly correlated one (AR(1), rho = 0.3: ~25 steps
            # instead of ~8) the conjugate gradients are REQUIRED to answer on register-resident systems and on bessx_cgbig's
            assert CG_REQUIRED.get((label, False), 0) >= 20 and CG_REQUIRED.get((label, True), 0) >= 4, CG_REQUIRED
        if not cg:  # with cov_solver=chol and in streaming mode CG never runs: the counter must say so
            assert s.counters()["cg_fallbacks"] == 0, "%s %s: %d Cholesky fallbacks" % (name, route, s.counters()["cg_fallbacks"])
    assert done == len(T0_SWEEP) * len(LAMS) * 2


@pytest.mark.parametrize("route", ["streaming", "cov"])
@pytest.mark.parametrize("name,weighted,fold", [("iid", True, -1), ("iid", False, 1), ("ar1", True, 1)])
def test_restricted_fits_with_weights_and_on_a_cv_fold(gpu, ref, monkeypatch, name, weighted, fold, route):
    mode, hk = ROUTES[route]
    if hk:
        hooks(monkeypatch, **hk)
    d = ref.design(name, weighted)
    with gpu.Session(d["X"], d["y"], weight=d["w"] if weighted else None, score_mode=mode) as s:
        if fold >= 0:
            s.set_cv(4, xprec.folds(s.n))
        cg = route == "cov"
        done = _sweep(ref, s, name, weighted, fold, "%s %s w=%d fold=%d" % (name, route, weighted, fold), must_cg=cg)
        assert cg or s.counters()["cg_fallbacks"] == 0
    assert done == len(T0_SWEEP) * len(LAMS) * 2


def test_cholesky_fallback_answers_on_the_collinear_design(gpu, ref, monkeypatch):
    """The reverse: the design and the call on which tests/test_cov_gpu.py already requires the Cholesky fallback to
    answer (6 clusters of 50 almost equal columns, the sequential path 1..24: conjugate gradients miss their residual
    target on some of its systems) -- here every candidate of that path is held to the bound, and the counter must say
    that Cholesky answered.  Single fits at 8, 12 and 24 columns come first: on them the conjugate gradients converge
    after all (few distinct eigenvalue clusters), which the sweep prints and nothing requires."""
    d = ref.design("collinear")
    n = d["Xs"].shape[0]
    t0s, seq = (8, 12, 24), np.arange(1, 25)
    with gpu.Session(d["X"], d["y"], score_mode=2) as s:
        done = _sweep(ref, s, "collinear", False, -1, "collinear cov", t0s)
        c0 = s.counters()["cg_fallbacks"]
        _, xn, _ = s.normalization()
        out = s.sequential_path(seq, ic_type=3)
        fell = s.counters()["cg_fallbacks"] - c0
        print("collinear path 1..24: %d Cholesky fallback(s)" % fell)
        assert fell > 0, "no system of the collinear path was handed to the Cholesky fallback"
        assert out["n_candidates"] == len(seq)
        for i, T0 in enumerate(seq):
            sup = out["cand_support"][i][:T0]
            assert np.all(sup >= 0) and len(np.unique(sup)) == T0 and np.all(out["cand_support"][i][T0:] == -1)
            b = xprec.ld(out["cand_beta"][i][:T0]) * xprec.ld(xn[sup]) / np.sqrt(LD(n))  # back to the normalised scale
            b_ref, condG = ref.fit("collinear", False, -1, None, 0.0, sup)
            what = "collinear path T0=%d" % T0
            _note("fit/bound collinear path", xprec.assert_fit_close(b, b_ref, condG, what))
            tr, _ = xprec.loss(d["Xs"], d["ys"], None, sup, b)
            _note("loss rel collinear path", xprec.assert_loss_close(out["cand_train_loss"][i], tr, what))
            done += 1
    hooks(monkeypatch, cov_solver="chol")
    with gpu.Session(d["X"], d["y"], score_mode=2) as s:
        done += _sweep(ref, s, "collinear", False, -1, "collinear cov-chol", t0s)
        assert s.counters()["cg_fallbacks"] == 0
    assert done == 2 * len(t0s) * len(LAMS) * 2 + len(seq)


def _required_cgbig_answer(s, T0, lam, condG, what):
    """A FRESH session queues CGB_GUESS_FIRST step launches per solve of its first large fit (the guess changes only at the
    end of a fit or after a fallback): where that many steps must suffice, bessx_cgbig.hip has to answer every system."""
    need = _cg_steps(COND_SLACK * condG)
    assert need <= CGB_GUESS_FIRST, "%s: cond %.3g needs up to %d steps, the test's design no longer guarantees a CG answer" % (
        what, condG, need)
    fell = s.counters()["cg_fallbacks"]
    assert fell == 0, "%s: bessx_cgbig.hip handed %d system(s) of cond %.3g (at most %d steps) to the blocked Cholesky" % (
        what, fell, condG, need)


@pytest.mark.parametrize("T0", [T0_FAST + 2, 420, 600])
def test_large_conjugate_gradients_answer_in_a_fresh_session(gpu, ref, T0):
    """bessx_cgbig.hip provably answers: first fit of a fresh session, ridge lam = n (the Gram's own scale: cond < 2.5, at
    most ~35 steps against the 40 queued), held to the same bounds, and not one system may go to the Cholesky fallback."""
    d = ref.design("iid")
    lam = float(d["Xs"].shape[0])
    with gpu.Session(d["X"], d["y"], score_mode=2) as s:
        r = s.fit(T0, lam, -1)
        what = "iid fresh session lam=n T0=%d" % T0
        _check_fit(ref, "iid", False, -1, None, lam, T0, r, what)
        _required_cgbig_answer(s, T0, lam, ref.fit("iid", False, -1, None, lam, r["support"])[1], what)


def test_hand_over_from_the_large_conjugate_gradients_to_the_blocked_cholesky(gpu, ref):
    """CGB_MAX_K and CGB_MAX_K + 1 in the covariance form, n >= 3 T0 (max_sparsity sizes the work space), ridge lam = 2 n so
    that the conjugate gradients at CGB_MAX_K provably answer within the fresh session's 40 step launches (cond ~2.1; at
    lam = 0 the cond ~14 of n = 3 T0 needs up to ~90).  CGB_MAX_K + 1 is the blocked Cholesky's directly: it adds no
    fallback (the counter counts systems the conjugate gradients gave up, and they are not asked)."""
    n, p = 3 * (CGB_MAX_K + 1) + 10, CGB_MAX_K + 1200
    X, y, _ = xprec.design_iid(n, p, 60, seed=105)
    Xs, ys = gpu.op_normalize(X, y, np.ones(n), 1, True, True)[:2]
    lam = 2.0 * n
    done = 0
    with gpu.Session(X, y, score_mode=2, max_sparsity=CGB_MAX_K + 1) as s:
        for T0 in LARGE_T0:
            r = s.fit(T0, lam, -1)
            sup = r["support"]
            assert len(sup) == T0 and len(np.unique(sup)) == T0
            b_ref, info = xprec.restricted_fit(Xs, ys, None, sup, lam)
            what = "large T0=%d" % T0
            _note("fit/bound " + what, xprec.assert_fit_close(r["beta"], b_ref, info["cond"], what))
            tr, _ = xprec.loss(Xs, ys, None, sup, r["beta"])
            _note("loss rel " + what, xprec.assert_loss_close(r["train_loss"], tr, what))
            if T0 == CGB_MAX_K:
                _required_cgbig_answer(s, T0, lam, info["cond"], what)
            else:
                assert s.counters()["cg_fallbacks"] == 0, "the blocked Cholesky's own level counted a fallback"
            done += 1
    assert done == len(LARGE_T0)


# ---- (b) the designs the suite lacked: tr / yy from 1e-3 through the guard at 1e-6 down to 1e-13 ---------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("level", xprec.SNR_LEVELS)
def test_losses_on_both_sides_of_the_guard(gpu, ref, level, mode):
    """The loss of the library's own coefficients, from fit and along a short sequential path (cand_train_loss; cand_ic
    recomputed from the reference loss).  The residual stays far above the rounding of y - X b (tr / yy ~ k u^2 ~ 1e-31 is
    where log(loss) becomes the reference's business)."""
    name = "snr%g" % level
    d = ref.design(name)
    n, p = d["Xs"].shape
    k = len(d["sup"])
    done = 0
    with gpu.Session(d["X"], d["y"], score_mode=mode) as s:
        r = s.fit(k, 0.0, -1)
        assert np.array_equal(r["support"], d["sup"]), "the true support is not recovered at tr/yy = %g" % level
        done += _check_fit(ref, name, False, -1, None, 0.0, k, r, "%s mode %d T0=%d fit" % (name, mode, k))
        yy = float(d["ys"] @ d["ys"]) / n
        print("%s mode %d: tr / yy = %.3e" % (name, mode, r["train_loss"] / yy))
        _, xn, _ = s.normalization()
        seq = [k - 2, k - 1, k, k + 1, k + 2]
        out = s.sequential_path(seq, ic_type=3)
        assert out["n_candidates"] == len(seq)
        for i, T0 in enumerate(seq):
            sup = out["cand_support"][i][:T0]
            assert np.all(sup >= 0) and np.all(out["cand_support"][i][T0:] == -1)
            b = xprec.ld(out["cand_beta"][i][:T0]) * xprec.ld(xn[sup]) / np.sqrt(LD(n))  # back to the normalised scale
            tr, _ = xprec.loss(d["Xs"], d["ys"], None, sup, b)
            what = "%s mode %d path T0=%d" % (name, mode, T0)
            _note("loss rel %s mode %d path" % (name, mode), xprec.assert_loss_close(out["cand_train_loss"][i], tr, what))
            want_ic = xprec.ic_value(tr, n, p, T0, 3)
            assert abs(out["cand_ic"][i] - want_ic) <= n * xprec.LOSS_RTOL + 1e-12 * abs(want_ic), (what, out["cand_ic"][i], want_ic)
            done += 1
    assert done == 1 + len(seq)


# ---- (c) scores ---------------------------------------------------------------------------------------------------------
def _gap_report(bd_ref, allowed_c1, T0, bd_lib, what):
    """Smallest score gap at the selection boundary next to the error the model allows there; the selection is asserted
    only where the gap exceeds it -- otherwise it is legitimately rounding-dependent."""
    order = np.argsort(-bd_ref.astype(np.float64), kind="stable")
    inside, outside = order[T0 - 1], order[T0]
    gap = float(bd_ref[inside] - bd_ref[outside])
    room = SCORE_C * float(allowed_c1[inside] + allowed_c1[outside])
    if gap > room:
        assert set(np.argsort(-bd_lib, kind="stable")[:T0]) == set(order[:T0]), what + ": selection differs from the reference's"
        print("%s: boundary gap %.3e > error bound %.3e: selection asserted" % (what, gap, room))
    else:
        print("%s: boundary gap %.3e <= error bound %.3e: the selection is rounding-dependent, not asserted" % (what, gap, room))


def _allowed_c1(r, form="cov"):
    S = r["S_cov"] if form == "cov" else r["S_stream"]
    phi, t = r["phi"].astype(np.float64), np.abs(r["t"].astype(np.float64))
    e = xprec.U * S / phi
    return 2 * t * e + e * e + xprec.U * t * t


@pytest.mark.parametrize("name", ["iid", "ar1"] + ["snr%g" % lv for lv in xprec.SNR_LEVELS])
def test_scores_inside_the_forward_error_model(gpu, ref, name):
    """(marginal_scores: host arithmetic on the device's x_j.y and x_j.x_j sums -- a check of those sums.)
    cov_state()[0] after a covariance-form fit against xprec.scores, and marginal_scores() (both modes) against the
    reference at beta = 0.  The scores in memory are those the fit's LAST iteration ranked: computed from the model of
    the iteration before (the trace has it), which on the normal end of a fit -- the active set repeated, the solve
    skipped -- is bitwise the returned model."""
    d = ref.design(name)
    k = len(d["sup"])
    done = 0
    r0 = xprec.scores(d["Xs"], d["ys"], None, [], [], 0.0, d["Xld"])
    with gpu.Session(d["X"], d["y"], score_mode=1) as s:
        ratio, j = xprec.score_error_units(s.marginal_scores(), r0, "cov")
        _note("score c marginal streaming", ratio)
        assert ratio <= SCORE_C, "%s marginal scores (streaming session): column %d needs c = %.1f" % (name, j, ratio)
        done += 1
    with gpu.Session(d["X"], d["y"], score_mode=2) as s:
        ratio, j = xprec.score_error_units(s.marginal_scores(), r0, "cov")
        _note("score c marginal cov", ratio)
        assert ratio <= SCORE_C, "%s marginal scores: column %d needs c = %.1f" % (name, j, ratio)
        done += 1
        s.trace_enable(True)
        for lam in LAMS:
            r = s.fit(k, lam, -1)
            f = s._trace()["fits"][-1]  # (capi offers the trace through path results only; a fit's is read this way)
            L = len(f["iters"])
            assert L >= 2, L  # (a fit always ranks at least twice: the all-zero start is column 0 of A_list)
            A, b = f["iters"][L - 2], f["betas"][L - 2]
            if np.array_equal(f["iters"][L - 1], A):  # normal end: the returned model is the scored one, bit for bit
                assert np.array_equal(r["support"], A) and np.array_equal(r["beta"], b)
            sr = xprec.scores(d["Xs"], d["ys"], None, A, b, lam, d["Xld"])
            bd = s.cov_state()[0]
            ratio, j = xprec.score_error_units(bd, sr, "cov")
            what = "%s scores after fit lam=%g" % (name, lam)
            print("%s: c = %.2f (column %d)" % (what, ratio, j))
            _note("score c after fit", ratio)
            assert ratio <= SCORE_C, "%s: column %d needs c = %.1f" % (what, j, ratio)
            _gap_report(sr["bd"], _allowed_c1(sr), k, bd, what)
            done += 1
    assert done == 2 + len(LAMS)


# ---- (d) Gram columns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", xprec.GRAM_SHAPES)
def test_gram_columns_of_the_prefill_route(gpu, ref, n, p):
    """cov_prefill_begin / compute / export on the large-mean, wide-scale design with non-unit weights: one group and a
    pair per pass where the column count allows.  (The export serves row set 0 of sessions without folds only.)"""
    X, y = xprec.design_large_mean(n, p)
    w = xprec.weights(n)
    Xs = gpu.op_normalize(X, y, w, 1, True, True)[0]
    ncol = min(128, p // 32 * 32)
    cols = ((np.arange(ncol) * 29 + 7) % p).astype(np.int32)
    want = xprec.gram_columns(Xs, None, cols)
    norms = np.sqrt((Xs * Xs).sum(axis=0))
    passes = {1: [(0, 1)], 3: [(0, 1), (1, 2)], 4: [(0, 1), (1, 1), (2, 2)]}[ncol // 32]
    with gpu.Session(X, y, weight=w, score_mode=2) as s:
        s.cov_prefill_begin(cols)
        for g0, ng in passes:
            s.cov_prefill_compute(g0, ng)
        got = s.cov_prefill_export(0, ncol // 32).reshape(ncol, p).T
        s.cov_prefill_end()
    f = xprec.assert_gram_close(got, want, norms[cols], norms, n, "Gram n=%d p=%d" % (n, p))
    _note("gram/bound", f)
    sub = got[cols, :]  # entry (a, b) = G[cols[a], cols[b]]: exported both ways
    assert np.array_equal(sub, sub.T), "exported Gram columns are not bitwise symmetric"


# ---- (e) normalisation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(130, 33), (1025, 129), (3001, 1100)])
def test_normalisation_of_large_means_and_wide_scales(gpu, ref, n, p):
    """bessx_op_normalize and Session.normalization() against the longdouble normalisation of the same inputs, fp64
    sources and -- through the device-input route -- fp32 sources whose values are exact in fp32."""
    import torch
    w = xprec.weights(n)
    for f32 in (False, True):
        X, y = xprec.design_large_mean(n, p, fp32_exact=f32)
        want = xprec.normalize(X, y, w, 1, True, True)
        Xs, ys, xm, xn, ym = gpu.op_normalize(X, y, w, 1, True, True)
        what = "n=%d p=%d %s" % (n, p, "fp32-exact" if f32 else "fp64")
        fc, fn = xprec.assert_normalization_close(Xs, xm, xn, want, w, "op_normalize " + what)
        _note("normalisation columns/tol", fc)
        _note("normalisation x_norm/tol", fn)
        assert abs(LD(ym) - want[4]) <= 4 * np.sqrt(n) * xprec.U * (abs(float(want[4])) + float(np.std(y)))
        src = torch.from_numpy(X.astype(np.float32)).cuda() if f32 else X
        with gpu.Session(src, y, weight=w, score_mode=2) as s:
            sm, sn, sy = s.normalization()
        # the session runs the kernel op_normalize runs: what (a)-(d) take as the library's own columns
        assert np.array_equal(sm, xm) and np.array_equal(sn, xn) and sy == ym, what + ": session differs from op_normalize"
        xprec.assert_normalization_close(Xs, sm, sn, want, w, "session " + what)
