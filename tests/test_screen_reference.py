"""CPU: the longdouble reference of the screening scores (tests/screenref.py) against fp64 NumPy on every case of
tests/test_screen_scores_gpu.py.  The fp64 stand-in takes the same number of steps everywhere and stays inside the
forward-error model (this is where SCREEN_C_LM / _LOGIT / _COX are measured); the reference alone meets the caps on
undecided and ill-conditioned units; the helper fails on a score that is wrong at 1e-9 relative, on a fit that took one
step more or fewer, and on each of four deliberately wrong forms of the reference (Newton clamp 30, the weight inside the
risk-set sums, the iterate after the last step, a suffix sum that restarts at row 256); where the compiled reference is
present, the kept sets the reference scores imply are its screening_A."""
import numpy as np
import pytest

import screenref as S
import xprec

pytestmark = pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format here")

FAMILIES = ("lm", "logistic", "cox")
_F64 = {}


def _standin(case):
    if case["name"] not in _F64:
        _F64[case["name"]] = S.reference(case, dtype=np.float64)
    return _F64[case["name"]]


def _case(name):
    fam = name.split("-")[0]
    return next(c for c in S.all_cases(fam) if c["name"] == name)


@pytest.mark.parametrize("family", FAMILIES)
def test_constants_are_the_rule_applied_to_the_measured_maxima(family):
    worst = (0.0, None)
    for case in S.all_cases(family):
        ref, f = S.cached_reference(case), _standin(case)
        assert np.array_equal(ref["steps"], f["steps"]), case["name"]  # fp64 and longdouble decide alike
        r, j = S.score_error_units(f["score"], ref)
        worst = max(worst, (r, "%s unit %d" % (case["name"], j)))
    recorded = {"lm": S.SCREEN_C_LM_NUMPY_MAX, "logistic": S.SCREEN_C_LOGIT_NUMPY_MAX, "cox": S.SCREEN_C_COX_NUMPY_MAX}[family]
    print("%s: fp64 NumPy scores at c = %.4f at %s (recorded %.4f, constant %g)" % (family, worst[0], worst[1], recorded,
                                                                               S.FAMILY_C[family]()))
    assert recorded / 1.001 <= worst[0] <= recorded * 1.0000001, worst  # the recorded maximum is the measured one
    assert S.FAMILY_C[family]() == S.constant_rule(recorded)


def test_the_reference_alone_meets_the_caps():
    total = bad = 0
    closest = np.inf
    for family in FAMILIES:
        for case in S.all_cases(family):
            ref = S.cached_reference(case)
            bad += S.assert_caps(ref, case, case["name"])
            total += ref["score"].size
            k = S.compared(ref)
            closest = min(closest, float(ref["margin"][k].min()))
            sc = ref["score"].astype(np.float64)
            # no compared unit has a bound above 1e-10 relative
            assert np.all(S.FAMILY_C[family]() * ref["unit_bound"][k] <= S.ILL_REL * sc[k]), case["name"]
            # the special columns are what the layout says
            if case["g_index"] is None:
                assert not ref["finite"][S.C_ZERO] and ref["always"][S.C_ALWAYS]
                assert ref["score"][S.C_DUP_A] == ref["score"][S.C_DUP_B]
                if family == "lm":
                    assert ref["score"][S.C_ZERO] == np.inf and ref["finite"][S.C_ONES]
                else:
                    assert not ref["finite"][S.C_ONES] and ref["score"][S.C_ONES] == 0.0 and ref["score"][S.C_ZERO] == 0.0
    print("%d of %d units undecided or ill-conditioned; closest compared decision %.2e from its threshold" % (bad, total, closest))
    assert bad <= 0.01 * total, (bad, total)
    assert closest >= S.MARGIN


def test_group_cases_hold_the_widths_on_both_sides_of_the_kernel_limits():
    for family, widths, limit in (("logistic", S.LOGIT_WIDTHS, 8), ("cox", S.COX_WIDTHS, 4)):
        for case in S.group_cases(family):
            sizes = np.diff(np.append(case["g_index"], case["X"].shape[1]))
            assert limit in sizes and limit + 1 in sizes and sizes.max() == 20, (case["name"], sizes)
            assert case["X"].shape[1] == sum(widths) + widths[0] and case["always"] == [sizes.size - 1]


PERTURB = ("lm-single-n257-plain-gauss", "logistic-single-n257-weighted-balanced", "cox-single-n257-weighted-cens30",
           "logistic-groups-n257-weighted-balanced", "cox-groups-n257-weighted-cens30")


@pytest.mark.parametrize("name", PERTURB)
def test_helper_fails_on_a_score_perturbed_by_1e_9(name):
    case = _case(name)
    ref = S.cached_reference(case)
    good = ref["score"].astype(np.float64)
    S.assert_scores_close(good, ref, name)
    S.assert_special_scores(good, ref, case, name)
    for u in np.nonzero(S.compared(ref))[0][[0, -1]]:
        bad = good.copy()
        bad[u] *= 1.0 + 1e-9
        with pytest.raises(AssertionError):
            S.assert_scores_close(bad, ref, name)
    # ... and the exact values: always_select, a degenerate unit, the duplicated pair
    bad = good.copy()
    bad[case["always"][0]] = 1e300
    with pytest.raises(AssertionError):
        S.assert_special_scores(bad, ref, case, name)
    if case["g_index"] is None:
        bad = good.copy()
        bad[S.C_ZERO] = 1e-300
        with pytest.raises(AssertionError):
            S.assert_special_scores(bad, ref, case, name)
        bad = good.copy()
        bad[S.C_DUP_B] = np.nextafter(bad[S.C_DUP_B], 1.0)
        with pytest.raises(AssertionError):
            S.assert_special_scores(bad, ref, case, name)


@pytest.mark.parametrize("name", [n for n in PERTURB if not n.startswith("lm")])
@pytest.mark.parametrize("delta", [-1, 1])
def test_helper_fails_on_a_fit_with_one_step_more_or_fewer(name, delta):
    case = _case(name)
    ref = S.cached_reference(case)
    units = S.unit_slices(case["X"].shape[1], case["g_index"])
    w = np.ones(case["X"].shape[0]) if case["weight"] is None else case["weight"]
    fit = S.logit_fit if case["family"] == "logistic" else S.cox_fit
    u = int(np.nonzero(S.compared(ref) & (ref["steps"] + delta >= 1) & (ref["steps"] + delta <= 30))[0][0])
    other = fit(case["X"][:, units[u]], case["y"], w, np.float64, force_stop=int(ref["steps"][u]) + delta)
    assert other["steps"] == ref["steps"][u] + delta
    scores = _standin(case)["score"].copy()
    S.assert_scores_close(scores, ref, name)
    scores[u] = other["score"]
    with pytest.raises(AssertionError):
        S.assert_scores_close(scores, ref, name)


WRONG = {"newton clamp 30": dict(newton_clamp=30.0), "weight in the risk-set sums": dict(weight_in_risk=True),
         "iterate after the last step": dict(after_last=True), "suffix sum restarts at row 256": dict(restart=256)}
# the cases each wrong form is shown on: the outlier column needs the clamp at 50; the weight needs a weighted case; the
# restart needs more than 256 rows
WRONG_CASES = ("cox-single-n257-weighted-cens90", "cox-single-n64-plain-cens30", "cox-groups-n257-weighted-cens30")


@pytest.mark.parametrize("what", sorted(WRONG))
def test_each_deliberately_wrong_reference_fails_the_comparison(what):
    """The stand-in plays the kernels; the comparison against a wrong reference must fail on at least one case."""
    failed = []
    for name in WRONG_CASES:
        case = _case(name)
        wrong = S.reference(case, **WRONG[what])
        try:
            S.assert_scores_close(_standin(case)["score"], wrong, "%s / %s" % (name, what))
        except AssertionError:
            failed.append(name)
    print(what, "fails on", failed)
    assert failed, what


def test_the_logistic_iterate_after_the_last_solve_fails_the_comparison():
    case = _case("logistic-single-n257-weighted-balanced")
    wrong = S.reference(case, after_last=True)
    with pytest.raises(AssertionError):
        S.assert_scores_close(_standin(case)["score"], wrong, case["name"])


ORACLE_CASES = {"lm": ("lm-single-n257-plain-gauss", "lm-single-n1000-weighted-gauss"),
                "logistic": ("logistic-single-n257-weighted-balanced", "logistic-groups-n257-weighted-balanced"),
                "cox": ("cox-single-n257-weighted-cens30", "cox-groups-n257-weighted-cens30")}


@pytest.mark.parametrize("family", FAMILIES)
def test_kept_sets_of_the_reference_scores_are_the_compiled_references(family):
    from oracle import ref_ctypes as R
    if not R.available():
        pytest.skip("the compiled reference is not present")
    for name in ORACLE_CASES[family]:
        case = _case(name)
        ref = S.cached_reference(case)
        keep = S.kept(ref["score"], case["screening_size"])
        assert keep is not None, name
        if case["g_index"] is None:
            got = R.screening(case["X"], case["y"], case["weight"], S.MODEL_TYPE[family], case["screening_size"],
                              case["always"])
        else:
            got = R.screening_groups(case["X"], case["y"], case["weight"], S.MODEL_TYPE[family], case["screening_size"],
                                     case["g_index"], case["always"])
        assert np.array_equal(np.sort(got), keep), (name, got, keep)
