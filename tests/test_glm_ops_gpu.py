"""GPU: the logistic and Poisson solver kernels, each called alone through the C ABI (bessx_op_glm_gh: k_glm_eta_gh, k_xtv,
k_score; bessx_op_glm_irls: k_irls_gram + k_gram_reduce, or k_glm_irls_prep + the Gram kernel, then k_chol), against the
longdouble reference of tests/glmref.py.  The bounds live in glmref.assert_*; tests/test_glm_reference.py shows on the CPU
that fp64 NumPy sits inside them (that is where their constants come from), that every helper fails on a result wrong at
1e-9, and that stand-ins of the defects this file exists for -- a dropped row pair at the end of a short slab, the working
response one Gram column early, the floor at t = 0, the 25 clamp in the training loss, the mask ignored in W -- fail.

(a) every template instance of the fused step at sparsity levels on and just past every tile-row edge, (b) slabs of several
chunks and several groups (rows_per_slab override) and the production geometry once per step of its rule, (c) both routes
on the saturating cases, against the reference and against each other, and the solve of the step on well-conditioned
systems of both families (bnext is compared only where the condition number is under glmref.COND_LIMIT), (d) op_glm_gh, (e) every call twice, bitwise the
same (inside (a) to (d)), (f) the loss a session's fit returns.

Not covered here: the convergence rule and the chain of steps (reached through Session.fit only: tests/test_glm_gpu.py and
the full-size golden tests), the pivoted fallback solve on a singular system, the screening kernels, the covariance-form
kernels.  (k_group_* are called alone in tests/test_group_ops_gpu.py.)

Measured on an MI355X (every test prints the fraction of each bound it uses, -s shows them): the file's 32 tests pass in
5.6 s.  Largest fraction of each bound used: g 0.134, h 0.131, loss 0.124, held-out loss 0.122, bd 0.187; Gram 0.108, ll
0.207, Wv 0.212, z 0.124, bnext 0.003; a slab override against the solver's geometry 0.011 of twice the Gram bound, the two
routes against each other 0.009 (Gram), 0.007 (ll), below 0.0005 (bnext); a session's train_loss 0.002.  No kernel had to
change.  The bounds do not depend on these figures: their constants come from fp64 NumPy on the CPU
(glmref.*_NUMPY_MAX), the rest is derived."""
import numpy as np
import pytest

import glmref as R
import xprec

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format")]

WORST = {}


def _note(**fracs):
    for k, v in fracs.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("largest fractions so far: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def _same(a, b):
    for k in a:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _step(gpu, family, case, **kw):
    """op_glm_irls twice: (e) bitwise the same."""
    X, y, w, mk, cols, bcur = case
    got = gpu.op_glm_irls(family, X, y, cols, bcur, weight=w, mask=mk, **kw)
    _same(got, gpu.op_glm_irls(family, X, y, cols, bcur, weight=w, mask=mk, **kw))
    return got


def _check_step(got, ref, what, lam=None):
    f = {"gram": R.assert_gram_close(got["gram"], ref, what), "ll": R.assert_ll_close(got["ll"], ref, what)}
    if got["wv"] is not None:
        f["wv"], f["z"] = R.assert_wv_close(got["wv"], ref, what), R.assert_z_close(got["z"], ref, what)
    if lam is not None:
        f["bnext"] = R.assert_bnext_close(got["bnext"], ref, lam, what)
    _note(**f)


# ---- (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T0", R.TEMPLATE_T0)
def test_fused_step_at_every_template_shape_and_tile_row_edge(gpu, T0):
    for family, t0, n, regime, t, wfloor, weighted, masked in R.template_cases():
        if t0 != T0:
            continue
        what = "fam%d T0=%d n=%d %s t=%d floor=%d w=%d m=%d" % (family, T0, n, regime, t, wfloor, weighted, masked)
        case = R.irls_case(family, T0, n, regime, weighted, masked)
        got = _step(gpu, family, case, route=1, t=t, wfloor=wfloor, want_bnext=False)
        assert got["route"] == 1 and got["wv"] is None
        _check_step(got, R.irls(family, *case, t, wfloor), what)


# ---- (b) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,T0", R.SLAB_T0)
def test_slabs_of_several_chunks_and_groups(gpu, nch, T0):
    """rows_per_slab = (NCH + 1) * 64: a full group of NCH chunks, then a one-chunk group whose registers were refilled
    under the products of the first; a short last slab with a ragged last chunk.  Within the bounds of the reference, and
    within twice the Gram bound of the solver's own geometry on the same input."""
    assert R.NCH_OF_MT[(T0 + 2 + 15) // 16] == nch
    rows = (nch + 1) * 64
    for family in (R.LOGISTIC, R.POISSON):
        for n, regime in [(n, r) for n in (R.slab_case_n(nch),) + ((1100,) if (nch, T0) == (8, 14) else ()) for r in R.SLAB_REGIMES]:
            what = "fam%d T0=%d n=%d rows_per_slab=%d %s" % (family, T0, n, rows, regime)
            case = R.irls_case(family, T0, n, regime, True, True, slab_rows=rows)
            ref = R.irls(family, *case, 1, 1)
            got = _step(gpu, family, case, route=1, t=1, wfloor=1, rows_per_slab=rows, want_bnext=False)
            _check_step(got, ref, what)
            own = _step(gpu, family, case, route=1, t=1, wfloor=1, want_bnext=False)
            _check_step(own, ref, what + " (64-row slabs)")
            _note(gram_geometries=R.assert_gram_close(got["gram"], ref, what + " against 64-row slabs", against=own["gram"], factor=2.0))


@pytest.mark.parametrize("family", (R.LOGISTIC, R.POISSON))
def test_production_slab_rule_past_16384_rows(gpu, family):
    """n = 16400: the row stride is 17408, irls_gram_slab_rows gives 128-row slabs, two chunks per block."""
    case = R.irls_case(family, 14, 16400, "saturating", True, True, slab_rows=128)
    got = _step(gpu, family, case, route=1, t=1, wfloor=1, want_bnext=False)
    _check_step(got, R.irls(family, *case, 1, 1), "fam%d T0=14 n=16400" % family)


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def _solved(family):
    """Is bnext compared on the saturating cases?  Logistic: W <= 1 / 4 whatever eta is, the systems stay well conditioned.
    Poisson: a row at e^30 beside rows at e^-12 puts the condition number past 1e13, where 4e-13 cond |b*| allows any
    vector (glmref.assert_bnext_close refuses such a case); there bnext only has to be finite and repeatable, and the solve
    is compared on glmref.SOLVE_CASES instead."""
    return family == R.LOGISTIC


def _check_routes(gpu, family, case, t, wfloor, lam, what, solved):
    ref = R.irls(family, *case, t, wfloor)
    five = _step(gpu, family, case, route=0, t=t, wfloor=wfloor, lam=lam)
    fused = _step(gpu, family, case, route=1, t=t, wfloor=wfloor, lam=lam)
    assert five["route"] == 0 and fused["route"] == 1 and five["wv"] is not None
    _check_step(five, ref, what + " five launches", lam if solved else None)
    _check_step(fused, ref, what + " fused", lam if solved else None)
    assert np.isfinite(five["bnext"]).all() and np.isfinite(fused["bnext"]).all(), what
    f = {"gram_routes": R.assert_gram_close(fused["gram"], ref, what + " fused against five launches", against=five["gram"], factor=2.0)}
    err, bound = abs(fused["ll"] - five["ll"]), 2 * R.SUM_C * ref["ll_bound"]
    assert err <= bound, (what, "ll of the two routes", fused["ll"], five["ll"], bound)
    f["ll_routes"] = err / bound if bound > 0 else 0.0
    if solved:
        cond = R.next_iterate(ref, lam)[1]
        assert cond <= R.COND_LIMIT, (what, cond)
        f["bnext_routes"] = xprec.assert_fit_close(fused["bnext"], five["bnext"], 2 * cond, what + " bnext of the two routes")
    _note(**f)
    assert _step(gpu, family, case, route=-1, t=t, wfloor=wfloor, lam=lam)["route"] == 1


@pytest.mark.parametrize("family", (R.LOGISTIC, R.POISSON))
@pytest.mark.parametrize("T0,n", ((14, 129), (30, 1025)))
def test_both_routes_on_the_saturating_cases(gpu, family, T0, n):
    case = R.irls_case(family, T0, n, "saturating", True, True)
    for t, wfloor in ((0, 1), (1, 1), (1, 0)):
        _check_routes(gpu, family, case, t, wfloor, 0.05, "fam%d T0=%d n=%d t=%d floor=%d" % (family, T0, n, t, wfloor), _solved(family))


@pytest.mark.parametrize("family", (R.LOGISTIC, R.POISSON))
def test_the_session_rule_takes_five_launches_past_eight_tile_rows(gpu, family):
    lam, T0, n = 0.05, 127, 1025
    case = R.irls_case(family, T0, n, "saturating", True, True)
    for t, wfloor in ((0, 1), (1, 1), (1, 0)):
        got = _step(gpu, family, case, route=-1, t=t, wfloor=wfloor, lam=lam)
        assert got["route"] == 0 and np.isfinite(got["bnext"]).all()
        _check_step(got, R.irls(family, *case, t, wfloor), "fam%d T0=127 n=%d t=%d floor=%d" % (family, n, t, wfloor),
                    lam if _solved(family) else None)
    with pytest.raises(gpu.BessxError):
        X, y, w, mk, cols, bcur = case
        gpu.op_glm_irls(family, X, y, cols, bcur, route=1)


@pytest.mark.parametrize("family", (R.LOGISTIC, R.POISSON))
@pytest.mark.parametrize("T0,n,regime", R.SOLVE_CASES)
def test_the_solve_of_the_step_on_well_conditioned_systems(gpu, family, T0, n, regime):
    """bnext of both routes (past eight tile rows: of the one a session takes) where 4e-13 cond |b*| is a statement about
    the solve: every case asserts that its condition number is under glmref.COND_LIMIT."""
    lam = 0.05
    case = R.irls_case(family, T0, n, regime, True, True)
    for t in (0, 1):
        what = "fam%d T0=%d n=%d %s t=%d" % (family, T0, n, regime, t)
        if T0 + 2 <= 128:
            _check_routes(gpu, family, case, t, 1, lam, what, True)
        else:
            got = _step(gpu, family, case, route=-1, t=t, wfloor=1, lam=lam)
            assert got["route"] == 0
            _check_step(got, R.irls(family, *case, t, 1), what, lam)


# ---- (d) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GH_N)
def test_gradient_curvature_losses_and_scores(gpu, n):
    for name, (family, case, lam) in R.all_gh_cases().items():
        X, y, w, mk, cols, b, coef0 = case
        if X.shape[0] != n:
            continue
        got = gpu.op_glm_gh(family, X, y, cols, b, coef0=coef0, lam=lam, weight=w, mask=mk)
        _same(got, gpu.op_glm_gh(family, X, y, cols, b, coef0=coef0, lam=lam, weight=w, mask=mk))
        ref = R.gh(family, *case)
        f = {"g": R.assert_g_close(got["g"], ref, name), "h": R.assert_h_close(got["h"], ref, name),
             "loss": R.assert_loss_close(got["loss"][0], ref, name),
             "bd": R.assert_scores_close(got["bd"], R.scores(X, ref, cols, b, lam), name)}
        if mk is not None:
            f["loss_test"] = R.assert_loss_close(got["loss"][1], ref, name, test=True)
        else:
            assert got["loss"][1] == 0.0
        _note(**f)


# ---- (f) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", (R.LOGISTIC, R.POISSON))
def test_the_loss_a_fit_returns_is_the_loss_of_its_coefficients(gpu, family):
    X, y = R.wide_design(family)
    with gpu.Session(X, y, data_type=2, model_type=family, is_normal=False) as s:
        got = s.fit(3)
    ref = R.gh(family, X, y, None, None, got["support"], got["beta"], got["coef0"])
    # train_loss = -2 x the sum of the summands: the bound of the sum, doubled (the product with -2 is exact)
    err, bound = float(abs(R.LD(got["train_loss"]) + 2 * ref["loss_all"])), 2 * R.SUM_C * ref["loss_all_bound"]
    print("fam%d: train_loss %.17g, |error| %.3e = %.3f of the bound; eta in [%.2f, %.2f]" % (
        family, got["train_loss"], err, err / bound, float(ref["eta"].min()), float(ref["eta"].max())))
    assert np.isfinite(got["train_loss"]) and err <= bound, (family, got["train_loss"], float(-2 * ref["loss_all"]), err, bound)
    assert float(ref["eta"].max()) - float(ref["eta"].min()) > 6.0, "the wide design no longer is"
    _note(session_loss=err / bound)
