"""GPU: the marginal-fit scores of screening, value by value (Session.screening_scores(): k_screen_score_lm,
k_screen_logit_pass, k_screen_logit_group, k_screen_cox, k_screen_cox_group of bessx_k_glm.hip, the sub-session route of
the wider groups and the device-matrix route), against the longdouble reference of tests/screenref.py under its
forward-error model: |score - score*| <= SCREEN_C_<family> x unit_bound on every compared unit, the exact values
(DBL_MAX, 0.0, +inf, the duplicated pair bitwise) on the special ones, and the reference's top-k as the kept set.
Sizes: one partial wave, the wave edge, the 256-row step of the block scans and strided sums with its carry (50, 64, 65,
255, 256, 257, 513, 1000); plain, weighted and with a tenth of the weights zero.

Measured on an MI355X, 2026-10-20, on top of commit 186909b (printed with -s by the last test of the file): the largest
|score - score*| / unit_bound was 1.077 for LM (lm-single-n50-weighted-gauss; allowed SCREEN_C_LM = 8), 0.852 for logistic
(logistic-single-n50-weighted-rare; allowed 32) and 18.169 for Cox (cox-single-n1000-plain-cens30, the outlier column whose
linear predictor passes 30; every other Cox case stayed below 0.33; allowed 32).  0 units undecided, 11 of 3656
ill-conditioned (all Cox noise columns: a mean of +-2 at a scale of 0.3 without an intercept cancels in x - S1 / S0).

What the first run of this file found: k_screen_logit_pass summed s0 as fma(W0, w, s0) but s1, s2 from the rounded W0 w,
and formed the determinant as fma(s0, s2, -(s1 s1)); an all-ones column (s0 = s1 = s2 by definition, slope 0 in the
reference) then scored anything from 0.056 to 5e24 in every WEIGHTED case and would have ranked first."""
import numpy as np
import pytest

import screenref as S
import xprec

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format")]

KW = {"lm": dict(), "logistic": dict(data_type=2, model_type=2), "cox": dict(data_type=3, model_type=4)}
_WORST = {}


def _names(cases):
    return [c["name"] for c in cases]


_CASES = {c["name"]: c for fam in ("lm", "logistic", "cox") for c in S.singleton_cases(fam) + S.group_cases(fam)}


def _session(gpu, case, X=None):
    kw = dict(KW[case["family"]])
    if case["g_index"] is not None:
        kw.update(g_index=case["g_index"], algorithm_type=2)
    return gpu.Session(case["X"] if X is None else X, case["y"], weight=case["weight"], is_screening=True,
                       screening_size=case["screening_size"], always_select=case["always"], **kw)


def _scores(gpu, case, X=None):
    with _session(gpu, case, X) as s:
        sc = s.screening_scores()
        keep = s.screening_groups() if case["g_index"] is not None else s.screening()
    assert sc.size == case["nunits"] and keep.size == case["screening_size"]
    return sc, keep


def _compare(gpu, name):
    case = _CASES[name]
    ref = S.cached_reference(case)
    sc, keep = _scores(gpu, case)
    S.assert_special_scores(sc, ref, case, name)
    r = S.assert_scores_close(sc, ref, name)
    fam = case["family"]
    _WORST[fam] = max(_WORST.get(fam, (0.0, None)), (r, name))
    want = S.kept(ref["score"], case["screening_size"])
    if want is not None:  # (None: the k-th and (k + 1)-th reference scores are too close to decide the top-k)
        assert np.array_equal(keep, want), (name, keep, want)


@pytest.mark.parametrize("name", _names(S.singleton_cases("lm")))
def test_lm_column_scores(gpu, name):
    """(x.y / x.x)^2 on the raw column; the weight does not enter (src/screening.cpp:46), so the weighted cases are held
    to the unweighted formula."""
    _compare(gpu, name)


@pytest.mark.parametrize("name", _names(S.singleton_cases("logistic")))
def test_logistic_column_scores(gpu, name):
    _compare(gpu, name)


@pytest.mark.parametrize("name", _names(S.singleton_cases("cox")))
def test_cox_column_scores(gpu, name):
    _compare(gpu, name)


@pytest.mark.parametrize("name", _names(S.group_cases("logistic")))
def test_logistic_group_scores(gpu, name):
    """Widths 1, 2, 3, 5, 8 | 9, 4, 20: the one-block kernel up to 8 columns and the sub-session fit from 9 on, held to one
    reference in the same call."""
    _compare(gpu, name)


@pytest.mark.parametrize("name", _names(S.group_cases("cox")))
def test_cox_group_scores(gpu, name):
    """Widths 1, 2, 3, 4 | 5, 20: the one-block kernel up to 4 columns and the sub-session fit from 5 on."""
    _compare(gpu, name)


@pytest.mark.parametrize("name", _names(S.group_cases("lm")))
def test_lm_group_scores_are_op_group_lsq(gpu, name):
    """The exported LM group scores are bitwise those of bessx_op_group_lsq on the same inputs (that kernel is pinned to
    its own longdouble reference in tests/test_group_ops_gpu.py)."""
    case = _CASES[name]
    sc, keep = _scores(gpu, case)
    want = gpu.op_group_lsq(case["X"], case["g_index"], case["y"], always=np.isin(np.arange(case["nunits"]), case["always"]))
    assert sc.tobytes() == want.tobytes(), (name, sc, want)
    assert sc[case["always"][0]] == S.DBL_MAX and case["always"][0] in keep


DEVICE_CASES = ("lm-single-n257-weighted-gauss", "lm-groups-n257-weighted-gauss", "logistic-single-n257-weighted-balanced",
                "logistic-groups-n257-weighted-balanced", "cox-single-n257-weighted-cens30",
                "cox-groups-n257-weighted-cens30")


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_scores_from_a_device_matrix_are_the_host_sessions(gpu, name):
    """X in GPU memory: an fp64 device matrix gives bitwise the host session's scores, an fp32 one bitwise those of a host
    session on X.astype(float32).astype(float64)."""
    torch = pytest.importorskip("torch")
    case = _CASES[name]
    host, keep = _scores(gpu, case)
    dev, dkeep = _scores(gpu, case, torch.from_numpy(case["X"]).cuda())
    assert dev.tobytes() == host.tobytes() and np.array_equal(keep, dkeep), name
    X32 = case["X"].astype(np.float32)
    host32, keep32 = _scores(gpu, case, X32.astype(np.float64))
    dev32, dkeep32 = _scores(gpu, case, torch.from_numpy(X32).cuda())
    assert dev32.tobytes() == host32.tobytes() and np.array_equal(keep32, dkeep32), name


def test_a_session_without_screening_has_no_scores(gpu):
    case = _CASES["lm-single-n50-plain-gauss"]
    with gpu.Session(case["X"], case["y"]) as s:
        assert s.screening_scores().size == 0


def test_zz_report_the_largest_bound_ratios(gpu):
    for fam in sorted(_WORST):
        print("%s: largest |score - score*| / unit_bound = %.3f at %s (allowed %g)"
              % (fam, _WORST[fam][0], _WORST[fam][1], S.FAMILY_C[fam]()))
