"""Cox residuals, dfbeta and case influence on an X already in GPU memory (bessx_cox_diag_device,
bess_amd/csrc/bessx_k_coxdiag.hip) against NumPy in np.longdouble on the host copy of the same values, within the bounds
derived in tests/coxdiagref.py at the device's addition depths.  Shapes: n = 1, 63, 1024 + 37 (two scan blocks with a
ragged tail), 2 * 1024 + 1 and one case of 5000 for the block-carry loop; m = 0, 1, 3, 4 (one k-step and its edge), 15, 16,
17 (tile edge), 33 and 65 (past a 64-column tile, a second run of output tiles).  Layouts: fp64 column-major, fp64
row-major, fp32 row-major and a view with both strides > 1, every element outside the view a NaN, the support scattered
over p = 300 columns.  dfbeta and displacement take an R and a C = R^T R of the test's own, given to both routes, so the
conditioning of an information matrix does not enter.  Layout, ties and weights cycle across the cases."""
import numpy as np
import pytest

import coxdiagref
import coxinforef
from bess_amd import capi, linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
KINDS = coxdiagref.KINDS
LAYOUTS = ["F", "C", "C32", "two_strides"]
TIES = ["order", "breslow"]
P = 300
NS, MS = (1, 63, 1024 + 37, 2 * 1024 + 1), (0, 1, 3, 4, 15, 16, 17, 33, 65)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _embed(layout, vals):
    """(base host array that holds vals in the layout under test, NaN everywhere else; base tensor -> the n x p view)"""
    n, p = vals.shape
    if layout in ("C", "C32"):  # row-major
        return vals.copy(), (lambda t: t)
    if layout == "F":  # column-major with a padded leading dimension: aligned columns, NaN rows >= n
        b = np.full((p, (n + 3) // 4 * 4), np.nan, dtype=vals.dtype)
        b[:, :n] = vals.T
        return b, (lambda t: t[:, :n].T)
    if layout == "two_strides":
        b = np.full((2 * n, 3 * p), np.nan, dtype=vals.dtype)
        b[::2, ::3] = vals
        return b, (lambda t: t[::2, ::3])
    raise AssertionError(layout)


_VALS, _PROBLEMS, _REFS, _TENSORS = {}, {}, {}, {}


def _vals(f32, n):
    if (f32, n) not in _VALS:
        _VALS[(f32, n)] = np.random.default_rng(5 * n + f32).standard_normal((n, P)).astype(np.float32 if f32 else np.float64)
    return _VALS[(f32, n)]


def _tensor(layout, n):
    """the device view of _vals under a layout, uploaded once"""
    if (layout, n) not in _TENSORS:
        base, view = _embed(layout, _vals(layout == "C32", n))
        _TENSORS[(layout, n)] = view(_dev(base))
    return _TENSORS[(layout, n)]


def _problem(f32, n, m):
    """One model per (dtype, n, m), the same logical values under every layout: beta ~ N(0, 1 / m), times on a grid of
    2.5 n points (about a third of the rows share one), about 70 % events, weights in eighths with zeros, and a lower
    triangular R of the size of an information factor with C = R^T R as fp64 data."""
    key = (f32, n, m)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + 7 * f32)
        cols = np.sort(rng.choice(P, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        time = rng.integers(0, int(2.5 * n) + 1, n) / 8.0
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0
        R = np.tril(rng.standard_normal((m, m))) / np.sqrt(max(n * m, 1)) + np.eye(m) / np.sqrt(n)
        _PROBLEMS[key] = dict(vals=_vals(f32, n), cols=cols, beta=beta, time=time, status=status, w=w, R=R, C=R.T @ R)
    return _PROBLEMS[key]


def _ref(pr, ties, w, time=None, status=None, key=None, beta=None):
    """coxdiagref.cox_diag_reference at the device's addition depths, once per distinct set of values"""
    if key is None or key not in _REFS:
        m = len(pr["cols"])
        ref = coxdiagref.cox_diag_reference(pr["vals"], pr["cols"], pr["beta"] if beta is None else beta,
                                            pr["time"] if time is None else time, pr["status"] if status is None else status,
                                            w, ties, pr["R"], pr["C"], coxdiagref.device_depths(m))
        if key is None:
            return ref
        _REFS[key] = ref
    return _REFS[key]


def _call(gpu, t, pr, ties, w, kinds=KINDS, time=None, status=None, beta=None):
    return gpu.cox_diagnostics_device(t, pr["cols"], pr["beta"] if beta is None else beta,
                                      pr["time"] if time is None else time, pr["status"] if status is None else status,
                                      factor=pr["R"], cinv=pr["C"], weight=w, ties=ties, kinds=kinds)


def _host(got):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_kind_is_within_the_bounds(gpu, layout, n):
    t = _tensor(layout, n)
    assert tuple(t.shape) == (n, P)
    f32 = int(layout == "C32")
    ni, li = NS.index(n), LAYOUTS.index(layout)
    for mi, m in enumerate(MS):
        pr = _problem(f32, n, m)
        ties, weighted = TIES[(mi + ni) % 2], (mi + ni + li) % 3 > 0
        # (device vectors for time / status / weight on every other case: they are copied to the host)
        dv = (mi + li) % 2 == 1
        w = pr["w"] if weighted else None
        ref = _ref(pr, ties, w, key=(f32, n, m, ties, weighted))
        got = gpu.cox_diagnostics_device(t, pr["cols"], pr["beta"], _dev(pr["time"]) if dv else pr["time"],
                                         _dev(pr["status"]) if dv else pr["status"], factor=pr["R"], cinv=pr["C"],
                                         weight=(_dev(w) if dv and weighted else w), ties=ties)
        what = "%s n=%d m=%d %s weighted=%s" % (layout, n, m, ties, weighted)
        J = int(pr["status"].sum())
        for k in KINDS:
            assert isinstance(got[k], torch.Tensor) and got[k].device == t.device and got[k].dtype == torch.float64, (what, k)
        assert tuple(got["score"].shape) == tuple(got["dfbeta"].shape) == (n, m), what
        assert tuple(got["schoenfeld"].shape) == (J, m) and tuple(got["displacement"].shape) == (n,), what
        print("%s: bL / mass %.3e" % (what, float(ref["rel"])))
        coxdiagref.check_cox_diag(_host(got), ref, KINDS, what)
        if m == 0:
            assert not got["displacement"].any().item(), what


def test_the_block_carry_loop(gpu):
    n, m = 5000, 33
    pr = _problem(0, n, m)
    for ties in TIES:
        got = _call(gpu, _tensor("F", n), pr, ties, pr["w"])
        coxdiagref.check_cox_diag(_host(got), _ref(pr, ties, pr["w"], key=(0, n, m, ties, True)), KINDS, "n=5000 " + ties)


@pytest.mark.parametrize("layout", ["F", "C32"])
def test_special_time_and_status_patterns(gpu, layout):
    """Distinct times in an order that is not the rows'; heavy ties (five distinct times) under both ties values; every
    time tied; no event (v = g = 0, L = 0, schoenfeld has no rows); every row an event; one event at the last position."""
    n, m = 1024 + 37, 17
    f32 = int(layout == "C32")
    pr = _problem(f32, n, m)
    t = _tensor(layout, n)
    rng = np.random.default_rng(19)
    last = np.zeros(n)
    last[n - 1] = 1.0
    five = np.round(rng.uniform(0, 4, n))
    cases = [("distinct", rng.permutation(n).astype(np.float64), pr["status"], "order"),
             ("five times", five, pr["status"], "order"), ("five times", five, pr["status"], "breslow"),
             ("all tied", np.full(n, 3.0), pr["status"], "breslow"), ("all tied", np.full(n, 3.0), pr["status"], "order"),
             ("no event", pr["time"], np.zeros(n), "breslow"), ("all events", pr["time"], np.ones(n), "breslow"),
             ("last only", np.arange(n, dtype=np.float64), last, "order")]
    for name, time, status, ties in cases:
        w = pr["w"] if name in ("five times", "all events") else None
        ref = _ref(pr, ties, w, time=time, status=status)
        got = _host(_call(gpu, t, pr, ties, w, time=time, status=status))
        coxdiagref.check_cox_diag(got, ref, KINDS, "%s %s %s" % (layout, name, ties))
        if name == "no event":
            assert not got["martingale"].any() and not got["deviance"].any() and not got["score"].any()
            assert not got["dfbeta"].any() and not got["displacement"].any() and got["schoenfeld"].shape == (0, m)
    assert len(np.unique(five)) == 5


def test_a_predictor_beyond_the_clamp(gpu):
    n, m = 1024 + 37, 4
    pr = _problem(0, n, m)
    beta = pr["beta"] * 40.0
    eta = pr["vals"][:, pr["cols"]] @ beta
    assert (eta > 30).any() and (eta < -30).any()
    for ties in TIES:
        ref = _ref(pr, ties, None, beta=beta)
        coxdiagref.check_cox_diag(_host(_call(gpu, _tensor("F", n), pr, ties, None, beta=beta)), ref, KINDS, "clamped " + ties)


def test_sums_agree_with_the_information_call(gpu):
    """Column sums of score against cox_information_device's score and sum martingale against its residual_sum;
    displacement against sum_c dfbeta * score; schoenfeld rows summed with weights wd against the score -- each within
    the summed bounds of both sides plus gamma_n of the summed magnitudes (coxdiagref item 18)."""
    n, m = 2 * 1024 + 1, 17
    pr = _problem(0, n, m)
    t = _tensor("F", n)
    for ties in TIES:
        ref = _ref(pr, ties, pr["w"], key=(0, n, m, ties, True))
        got = _host(_call(gpu, t, pr, ties, pr["w"]))
        info = gpu.cox_information_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], weight=pr["w"], ties=ties)
        J = int(pr["status"].sum())
        iref = coxinforef.cox_information_reference(pr["vals"], pr["cols"], pr["beta"], pr["time"], pr["status"], pr["w"],
                                                    ties, coxinforef.device_depths(gpu, n, m, J))
        gn, gm = coxdiagref.gamma(n), coxdiagref.gamma(m + 1)
        sL, bL = np.abs(ref["score"]), ref["score_bound"]
        err = np.abs(got["score"].sum(axis=0).astype(LD) - info["score"].astype(LD))
        bound = bL.sum(axis=0) + gn * (sL + bL).sum(axis=0) + iref["score_bound"]
        print("%s: column sums err %.3e bound %.3e" % (ties, float(err.max()), float(bound.min())))
        assert (err <= bound).all()
        err = abs(LD(got["martingale"].sum()) - LD(info["residual_sum"]))
        bound = ref["martingale_bound"].sum() + gn * (np.abs(ref["martingale"]) + ref["martingale_bound"]).sum() + \
            iref["residual_bound"]
        assert err <= bound, (float(err), float(bound))
        # displacement = L C L^T with C = R^T R; the C both routes are given is that product rounded in fp64
        sD, bD = np.abs(ref["dfbeta"]), ref["dfbeta_bound"]
        cross = (got["dfbeta"] * got["score"]).sum(axis=1).astype(LD)
        bound = ref["displacement_bound"] + (sD * bL + sL * bD + bL * bD).sum(axis=1) + gm * ((sD + bD) * (sL + bL)).sum(axis=1)
        bound = bound + gm * ((sL @ np.abs(pr["R"]).T.astype(LD)) ** 2).sum(axis=1)
        err = np.abs(got["displacement"].astype(LD) - cross)
        print("%s: displacement against dfbeta . score err %.3e bound %.3e" % (ties, float(err.max()), float(bound.min())))
        assert (err <= bound).all()
        wd = ref["wd"][ref["event_rows"]]
        ssum = (got["schoenfeld"].astype(LD) * wd[:, None]).sum(axis=0)
        gj = coxdiagref.gamma(J + 1)
        bound = (wd[:, None] * ref["schoenfeld_bound"]).sum(axis=0) + gj * (
            wd[:, None] * (np.abs(ref["schoenfeld"]) + ref["schoenfeld_bound"])).sum(axis=0) + iref["score_bound"]
        err = np.abs(ssum - info["score"].astype(LD))
        assert (err <= bound).all(), (float(err.max()), float(bound.min()))


def test_layouts_of_one_dtype_agree(gpu):
    """A column-major X and a view with both strides > 1 take the same kernels in the same order: the same bits.  A
    row-contiguous X is served by another loop of the predictor pass this call reuses (k_xb_gather adds the support's
    products in another order), so e differs in its last bits and everything after it: there the two layouts are held
    to each other within the sum of their bounds."""
    n, m = 1024 + 37, 33
    pr = _problem(0, n, m)
    ref = _ref(pr, "breslow", pr["w"], key=(0, n, m, "breslow", True))
    res = {lay: _host(_call(gpu, _tensor(lay, n), pr, "breslow", pr["w"])) for lay in ("F", "two_strides", "C")}
    for k in KINDS:
        assert np.array_equal(res["F"][k], res["two_strides"][k]), k
        err = np.abs(res["F"][k].astype(LD) - res["C"][k].astype(LD))
        assert (err <= 2 * ref[k + "_bound"]).all(), k


def test_requests_repeat_and_device_memory_is_given_back(gpu):
    n, m = 2 * 1024 + 1, 33
    pr = _problem(0, n, m)
    t = _tensor("C", n)
    before = gpu.process_counters()
    runs = []
    counters = []
    for _ in range(3):
        runs.append(_host(_call(gpu, t, pr, "breslow", pr["w"])))
        counters.append(gpu.process_counters())
    for k in KINDS:
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k], runs[2][k]), k
    for c in counters:
        assert c["live_device_bytes"] == before["live_device_bytes"]
        assert c["live_pinned_bytes"] == before["live_pinned_bytes"]
    added = counters[1]["allocation_requests"] - counters[0]["allocation_requests"]
    assert added > 0 and counters[2]["allocation_requests"] - counters[1]["allocation_requests"] == added
    # martingale and deviance alone form no gather, no U and no A: fewer requests
    _call(gpu, t, pr, "breslow", pr["w"], kinds=("martingale", "deviance"))
    small = gpu.process_counters()
    assert 0 < small["allocation_requests"] - counters[2]["allocation_requests"] < added
    assert small["live_device_bytes"] == before["live_device_bytes"]
    # a NumPy result for a device object that is not a torch tensor, the same bits
    class View:
        def __init__(self, t):
            self.__cuda_array_interface__ = t.__cuda_array_interface__
    got = _call(gpu, View(t), pr, "breslow", pr["w"])
    for k in KINDS:
        assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], runs[0][k]), k


def test_the_estimator_on_a_device_matrix(gpu):
    """est.diagnostics_survival(X_dev, y) against the NumPy route on the host copy.  The kinds that do not involve the
    inverse information agree within the sum of the two routes' bounds.  dfbeta and displacement take each route's own
    factor (of that route's own information matrix, which differ in their last bits), so each route is held to the
    reference formed with the R and C that route used."""
    n, m = 1024 + 37, 4
    pr = _problem(0, n, m)
    beta = np.zeros(P)
    beta[pr["cols"]] = pr["beta"]
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = P, beta, 0.0
    y = np.column_stack([pr["time"], pr["status"]])
    t = _tensor("C", n)
    w = np.ones(n)
    for ties in TIES:
        dev = est.diagnostics_survival(t, _dev(y), weight=pr["w"], ties=ties)
        host = est.diagnostics_survival(pr["vals"], y, weight=pr["w"], ties=ties)
        assert dev["positive_definite"] and host["positive_definite"] and np.array_equal(dev["cols"], pr["cols"])
        for route, got, depths in (("device", _host(dev), coxdiagref.device_depths(m)), ("host", host, coxdiagref.host_depths(m))):
            if route == "device":
                info = gpu.cox_information_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], weight=pr["w"],
                                                  ties=ties)["info"]
            else:
                info = linear.bess_base._cox_information_host(pr["vals"][:, pr["cols"]], pr["beta"], pr["time"],
                                                              pr["status"], pr["w"], ties)["info"]
            R, pd = capi.info_factor(info)
            ref = coxdiagref.cox_diag_reference(pr["vals"], pr["cols"], pr["beta"], pr["time"], pr["status"], pr["w"], ties,
                                                R, R.T @ R, depths)
            coxdiagref.check_cox_diag(got, ref, KINDS, "estimator %s %s" % (route, ties))
            if route == "device":
                dref = ref
        for k in ("martingale", "deviance", "score", "schoenfeld"):
            err = np.abs(_host(dev)[k].astype(LD) - host[k].astype(LD))
            assert (err <= dref[k + "_bound"] + ref[k + "_bound"]).all(), k
        tb = est.inference_survival(t, y, weight=pr["w"], ties=ties)
        assert dev["loglik"] == tb["loglik"] and dev["residual_sum"] == tb["residual_sum"]
        assert np.array_equal(dev["event_rows"], host["event_rows"]) and np.array_equal(dev["event_times"], host["event_times"])
    assert est.diagnostics(t, y) is None
    del w


def test_argument_errors_on_the_device(gpu):
    n, m = 63, 3
    pr = _problem(0, n, m)
    t = _tensor("F", n)
    with pytest.raises(gpu.BessxError, match="dfbeta needs cinv"):
        gpu.cox_diagnostics_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], factor=pr["R"])
    with pytest.raises(gpu.BessxError, match="the lower triangle of the factor must be finite"):
        gpu.cox_diagnostics_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], factor=np.full((m, m), np.nan),
                                   kinds="displacement")
    # the strict upper triangle of the factor is not read
    R = pr["R"] + np.triu(np.full((m, m), np.nan), 1)
    a = gpu.cox_diagnostics_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], factor=R, kinds="displacement")
    b = gpu.cox_diagnostics_device(t, pr["cols"], pr["beta"], pr["time"], pr["status"], factor=pr["R"], kinds="displacement")
    assert torch.equal(a["displacement"], b["displacement"])
