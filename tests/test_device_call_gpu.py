"""Every entry point that takes a caller's X in GPU memory (include/bessx.h sections 2c to 2o), at one small shape: the
call with y / weight (Cox: time / status / weight; the meat: u) in host memory and the call with the same values in
GPU memory give the same bits, and after each call the library holds exactly the device and pinned bytes it held
before it -- whatever a call allocates for itself goes when the call returns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, P, M = 64, 8, 2
COLS = np.array([1, 5], dtype=np.int32)
CAND = [0, 2, 3, 7]          # 4 tested columns
STARTS, GROUPS = [0, 2, 4, 6], [1, 3]  # 2 tested groups of 2 columns


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_DATA = {}


def _data():
    if not _DATA:
        rng = np.random.default_rng(20)
        X = rng.standard_normal((N, P))
        beta = np.array([0.4, -0.3])
        _DATA.update(X=X, x=_dev(X), beta=beta, coef0=0.2, y=(rng.uniform(size=N) < 0.5).astype(float),
                     w=rng.integers(1, 9, N) / 8.0, time=np.floor(rng.uniform(0, 20, N)),  # (tied times)
                     status=(rng.uniform(size=N) < 0.7).astype(float), u=rng.standard_normal(N))
    return _DATA


def _glm(call):
    return lambda capi, d, y, w: call(capi, d["x"], COLS, d["beta"], d["coef0"], y, w)


def _cox(call):
    return lambda capi, d, t, s, w: call(capi, d["x"], COLS, d["beta"], t, s, w)


def _survival(capi, d, t, s, w):
    base = capi.cox_baseline_device(d["x"], COLS, d["beta"], t, s, weight=w)
    return {"curves": capi.cox_survival_device(d["x"], COLS, d["beta"], base["times"], base["cumhaz"]), **base}


# name -> (the data arguments that go once as host and once as device arrays, the call)
GLM_CALLS = {
    "evaluate": _glm(lambda c, x, cols, b, c0, y, w: c.evaluate_device(x, cols, b, [c0], y, link="logistic", weight=w)),
    "information": _glm(lambda c, x, cols, b, c0, y, w: c.information_device(x, cols, b, c0, y, link="logistic", weight=w)),
    "diagnostics": _glm(lambda c, x, cols, b, c0, y, w: c.diagnostics_device(
        x, cols, b, c0, y, factor=c.info_factor(c.information_device(x, cols, b, c0, y, link="logistic", weight=w)["info"])[0],
        link="logistic", weight=w)),
    "sandwich": _glm(lambda c, x, cols, b, c0, y, w: c.sandwich_device(x, cols, b, c0, y, link="logistic", weight=w,
                                                                      cluster=np.arange(N) // 4)),
    "addscore": _glm(lambda c, x, cols, b, c0, y, w: c.addscore_device(x, cols, b, c0, y, link="logistic", weight=w,
                                                                      candidates=CAND, want_cross=True)),
    "groupscore": _glm(lambda c, x, cols, b, c0, y, w: c.groupscore_device(x, cols, b, c0, y, STARTS, groups=GROUPS,
                                                                          link="logistic", weight=w)),
}
COX_CALLS = {
    "evaluate_cox": _cox(lambda c, x, cols, b, t, s, w: c.evaluate_cox_device(x, cols, b, t, s, weight=w, ties="breslow")),
    "cox_baseline_and_survival": _survival,
    "cox_information": _cox(lambda c, x, cols, b, t, s, w: c.cox_information_device(x, cols, b, t, s, weight=w,
                                                                                  ties="breslow")),
    "cox_diagnostics": _cox(lambda c, x, cols, b, t, s, w: c.cox_diagnostics_device(
        x, cols, b, t, s, weight=w, ties="breslow", kinds=("martingale", "deviance", "score", "schoenfeld"))),
    "cox_addscore": _cox(lambda c, x, cols, b, t, s, w: c.cox_addscore_device(x, cols, b, t, s, weight=w, ties="breslow",
                                                                             candidates=CAND, want_cross=True)),
    "cox_groupscore": _cox(lambda c, x, cols, b, t, s, w: c.cox_groupscore_device(x, cols, b, t, s, STARTS, groups=GROUPS,
                                                                                 weight=w, ties="breslow")),
}


def _host(v):
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy()
    if isinstance(v, tuple):
        return tuple(_host(t) for t in v)
    return v


def _same_bits(a, b, what):
    a, b = _host(a), _host(b)
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same_bits(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, tuple):
        for k, (s, t) in enumerate(zip(a, b)):
            _same_bits(s, t, "%s[%d]" % (what, k))
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    else:
        assert a == b or (a != a and b != b), what


def _counted(capi, call):
    """The result of call(); the library's device and pinned bytes are back where they were."""
    before = capi.process_counters()
    got = call()
    after = capi.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"], (before, after)
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"], (before, after)
    assert after["allocation_requests"] > before["allocation_requests"]  # (the call did go through the owners)
    return got


@pytest.mark.parametrize("name", sorted(GLM_CALLS))
def test_glm_host_and_device_data_give_the_same_bits_and_nothing_stays_allocated(gpu, name):
    d, call = _data(), GLM_CALLS[name]
    host = _counted(gpu, lambda: call(gpu, d, d["y"], d["w"]))
    dev = _counted(gpu, lambda: call(gpu, d, _dev(d["y"]), _dev(d["w"])))
    _same_bits(host, dev, name)
    assert all(np.isfinite(_host(v)).all() for v in host.values() if isinstance(_host(v), np.ndarray)), name


@pytest.mark.parametrize("name", sorted(COX_CALLS))
def test_cox_host_and_device_data_give_the_same_bits_and_nothing_stays_allocated(gpu, name):
    d, call = _data(), COX_CALLS[name]
    host = _counted(gpu, lambda: call(gpu, d, d["time"], d["status"], d["w"]))
    dev = _counted(gpu, lambda: call(gpu, d, _dev(d["time"]), _dev(d["status"]), _dev(d["w"])))
    _same_bits(host, dev, name)


def test_predict_and_meat_leave_nothing_allocated(gpu):
    d = _data()
    pr, lab = _counted(gpu, lambda: gpu.predict_device(d["x"], COLS, d["beta"], [d["coef0"]], link="logistic"))
    eta = d["X"][:, COLS] @ d["beta"] + d["coef0"]
    assert _host(lab).shape == (N,) and np.allclose(_host(pr), 1 / (1 + np.exp(-eta)), rtol=1e-12, atol=0)
    host = _counted(gpu, lambda: gpu.meat_device(d["x"], COLS, u=d["u"], cluster=np.arange(N) // 4))
    dev = _counted(gpu, lambda: gpu.meat_device(d["x"], COLS, u=_dev(d["u"]), cluster=_dev(np.arange(N) // 4)))
    _same_bits(host, dev, "meat")
