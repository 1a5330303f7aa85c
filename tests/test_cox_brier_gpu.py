"""The IPCW Brier score on an X already in GPU memory (bessx_cox_brier_device, bess_amd/csrc/bessx_k_coxbrier.hip)
against NumPy in np.longdouble on the host copy of the same (widened) values.  The bound is derived in tests/coxbrierref.py,
which also asserts for every input here that the bound is below 1e-9 of the score; every check prints error against bound
for every entry.  The shapes are the smallest that reach every path of the kernels as built: CXB_ROWS = 1024 rows per slab
(n = 1, 1023, 1024, 1025 and two slabs plus one, 2049), CXB_T = 256 threads regrouped into 256 / TJ row groups of TJ lanes
for T <= 256 times (T = 1: 256 groups of one lane, T = 2, T = 7: 32 groups of 8, T = 100: 2 groups of 128 with idle
lanes) and chunks of 256 times beyond (T = 255, 256, 257 and two chunks plus one, 513), R = 1 and 3 models (one grid row
each; the predictor pass has a kernel for R = 1 and one for R <= 4), supports of m = 0, 1 and 65 columns (both branches of
the predictor's chunk loop) and the four layouts of tests/test_cox_surv_gpu.py."""
import ctypes

import numpy as np
import pytest

import coxbrierref
import coxsurvref
import evalref
from bess_amd import linear, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
U = evalref.U
P = 80
NMAX = 2049
_REFS = {}
_BT = 0.3 + np.cumsum(np.random.default_rng(11).uniform(0.01, 0.2, 40))  # (every row time below 0.3 meets hg = 0)
_BH = np.cumsum(np.random.default_rng(12).uniform(0.0, 0.1, 40))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _problem(n, m, R=3, seed=91):
    """X (n x P, N(0, 1)), m ascending support columns, R models with coefficients N(0, 1 / m) (|eta| stays below 5),
    continuous times in an order that is not the rows', about 60% events."""
    rng = np.random.default_rng(seed + 7 * m)
    X = rng.standard_normal((NMAX, P))[:n]
    cols = np.sort(rng.choice(P, m, replace=False)).astype(np.int32)
    B = rng.standard_normal((m, 3))[:, :R] / np.sqrt(max(m, 1))
    time = rng.exponential(1.0, NMAX)[:n] + 0.05
    status = (rng.uniform(size=NMAX) < 0.6).astype(np.float64)[:n]
    return X, cols, B, time, status


def _weights(n, kind):
    if kind == "none":
        return None
    w = np.random.default_rng(5).integers(1, 17, NMAX)[:n] / 8.0
    if kind == "zeros":
        w[::3] = 0.0
        w[0] = 1.0
    return w


LAYOUTS = ["f64 row-major", "f64 column-major", "f32 row-major", "strided"]


def _view(vals, layout):
    """(the n x P device view of the values in the given layout, the widened values it holds)"""
    n, p = vals.shape
    if layout == "f64 row-major":
        return _dev(vals), vals
    if layout == "f64 column-major":
        F = np.full((p, (n + 3) // 4 * 4), np.nan)
        F[:, :n] = vals.T
        return _dev(F)[:, :n].T, vals
    if layout == "f32 row-major":
        v32 = vals.astype(np.float32)
        return _dev(v32), v32.astype(np.float64)
    S = np.full((2 * n, 3 * p), np.nan)  # both strides > 1
    S[::2, 1::3] = vals
    return _dev(S)[::2, 1::3], vals


def _eta(key, vals, cols, B):
    if key not in _REFS:
        _REFS[key] = evalref.eta_reference(vals, cols, B, np.zeros(np.shape(B)[1]))
    return _REFS[key]


def _last_admissible(time, status, w):
    """The largest time at which the Kaplan-Meier censoring estimate of the rows is positive (the last row time, or the
    float below it when a row of positive weight is censored there)."""
    top = time.max()
    wl = np.ones(time.size) if w is None else w
    return np.nextafter(top, -np.inf) if ((time == top) & (status == 0) & (wl > 0)).any() else top


def _times(time, status, w, T, seed=0):
    """T ascending distinct times: below the smallest row time, equal to row times, between them, and (last) the largest
    admissible one."""
    rng = np.random.default_rng(seed + T)
    u = np.unique(time)
    last = _last_admissible(time, status, w)
    if T == 1:
        return np.array([u[u.size // 2]])
    must = [0.5 * u[0], last] + list(u[:-1][rng.permutation(u.size - 1)[:max(min(T // 3, u.size - 1), 0)]])
    for _ in range(8):
        g = np.unique(np.concatenate([must, rng.uniform(u[0], last, max(T - len(must), 0))]))
        g = g[g <= last]
        if g.size >= T:
            keep = np.sort(rng.permutation(g.size - 2)[:T - 2] + 1) if T > 2 else np.array([], dtype=np.int64)
            return g[np.concatenate([[0], keep, [g.size - 1]]).astype(np.int64)]
    return g  # (n = 1: fewer than T distinct times exist)


def _hg(times, R):
    """(T, R): a step-function baseline at the times, a different multiple of it per model; 0 before its first time."""
    from bess_amd import capi
    base = capi.baseline_at(_BT, _BH, times)
    return np.column_stack([base * (1.0 + 0.5 * r) for r in range(R)])


def _check(gpu, t, eta, delta, cols, B, hg, times, time, status, w, censoring, what, ipcw=True):
    n, T, R = time.size, times.size, np.shape(B)[1]
    got = gpu.cox_brier_device(t, cols, B, hg, times, time, status, weight=w, censoring=censoring)
    assert set(got) == {"brier", "null", "ipa", "ibs", "ibs_null", "row_a", "time_b", "sum_w"}
    assert got["brier"].shape == (T, R) and got["ipa"].shape == (T, R) and got["null"].shape == (T,)
    assert got["ibs"].shape == (R,)
    a, b = got["row_a"], got["time_b"]
    if censoring == "km" and ipcw:
        coxbrierref.check_ipcw(a, b, coxbrierref.ipcw_reference(time, status, times, w), n, what)
    ref = coxbrierref.brier_reference(eta, delta, hg, times, time, w, a, b, coxbrierref.device_depth(n, T), what)
    coxbrierref.check_brier(got["brier"], ref, what)
    wl = np.ones(n) if w is None else w
    assert abs(LD(got["sum_w"]) - wl.astype(LD).sum()) <= evalref.gamma(n) * wl.sum()
    want = gpu._brier_result(got["brier"], times, time, status, wl, a, b)  # the host's part, from the same scores
    for k in ("null", "ipa", "ibs"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    if T >= 2 and (np.diff(times) > 0).all():
        assert np.array_equal(got["ibs"], gpu.integrated_brier(times, got["brier"]))
    else:
        assert np.isnan(got["ibs"]).all() and np.isnan(got["ibs_null"])
    return got, ref


# ----------------------------------------------------------------------------------------------------------------
# the shapes
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_the_row_slab_edges_with_every_kind_of_weight_and_censoring(gpu, n):
    T, R, m = 7, 3, 3
    X, cols, B, time, status = _problem(n, m)
    if n == 1:
        status = np.ones(1)
    assert gpu.cox_brier_workspace(n, T, R)[1:] == (coxbrierref.SLAB_ROWS, -(-n // 1024), coxbrierref.row_groups(T))
    assert coxbrierref.row_groups(T) == 32
    t = _dev(X)
    eta, delta = _eta(("slab", n), X, cols, B)
    for wk in ("none", "eighths", "zeros"):
        w = _weights(n, wk)
        times = _times(time, status, w, T)
        hg = _hg(times, R)
        for censoring in ("km", None, "given"):
            cens = censoring
            if censoring == "given":
                cens = (np.random.default_rng(3).uniform(0.0, 2.0, n) * status, np.linspace(1.0, 3.0, times.size))
            got, _ = _check(gpu, t, eta, delta, cols, B, hg, times, time, status, w, cens,
                            "n=%d w=%s censoring=%s" % (n, wk, censoring))
            if censoring is None:
                assert np.array_equal(got["row_a"], status) and (got["time_b"] == 1.0).all()
            if censoring == "given":
                assert np.array_equal(got["row_a"], cens[0]) and np.array_equal(got["time_b"], cens[1])


@pytest.mark.parametrize("T,R", [(1, 3), (2, 1), (100, 3), (255, 1), (256, 1), (257, 1), (513, 1)])
def test_the_lane_groupings_and_the_time_chunk_edges(gpu, T, R):
    n, m = 1025, 3
    X, cols, B, time, status = _problem(n, m, R)
    assert gpu.cox_brier_workspace(n, T, R)[3] == {1: 256, 2: 128, 100: 2}.get(T, 1)
    eta, delta = _eta(("chunk", R), X, cols, B)
    w = _weights(n, "eighths")
    times = _times(time, status, w, T)
    assert times.size == T
    t = _dev(X)
    got, ref = _check(gpu, t, eta, delta, cols, B, _hg(times, R), times, time, status, w, "km", "T=%d R=%d" % (T, R))
    again = gpu.cox_brier_device(t, cols, B, _hg(times, R), times, time, status, weight=w)
    assert np.array_equal(_bits(again["brier"]), _bits(got["brier"]))  # the same call gives the same bits
    if T == 100:  # the times in any order, with repeats (another lane grouping: its own reference), no integral
        pick = np.random.default_rng(1).integers(0, T, 37)
        _check(gpu, t, eta, delta, cols, B, _hg(times[pick], R), times[pick], time, status, w, "km", "T=37, unsorted")
        one = gpu.cox_brier_device(t, cols, B[:, 1], _hg(times, R)[:, 1], times, time, status, weight=w)  # 1-D B and hg
        assert one["brier"].shape == (T, 1) and one["ibs"].shape == (1,)
        assert (np.abs(one["brier"][:, 0].astype(LD) - ref["value"][:, 1]) <= ref["bound"][:, 1]).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_layout_of_x_and_every_support_size(gpu, layout):
    n, T, R = 1025, 5, 3
    for m in (0, 1, 65):
        X, cols, B, time, status = _problem(n, m)
        t, vals = _view(X, layout)
        assert tuple(t.shape) == (n, P)
        keep = t.clone()
        eta, delta = _eta(("layout", m, layout == "f32 row-major"), vals, cols, B)
        times = _times(time, status, None, T)
        before = gpu.process_counters()
        got, _ = _check(gpu, t, eta, delta, cols, B, _hg(times, R), times, time, status, None, "km",
                        "%s m=%d" % (layout, m), ipcw=False)
        after = gpu.process_counters()
        assert after["live_device_bytes"] == before["live_device_bytes"]
        assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
        assert torch.equal(t, keep)  # x is never written
        again = gpu.cox_brier_device(t, cols, B, _hg(times, R), times, time, status)
        assert np.array_equal(_bits(again["brier"]), _bits(got["brier"]))


# ----------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------
def _common():
    if "common" not in _REFS:
        X, cols, B, time, status = _problem(1025, 3)
        _REFS["common"] = (X, cols, B, time, status) + tuple(_eta(("common",), X, cols, B))
    return _REFS["common"]


def test_every_row_censored_leaves_only_the_b_term(gpu):
    X, cols, B, time, _, eta, delta = _common()
    n, status = time.size, np.zeros(time.size)
    for wk in ("none", "zeros"):
        w = _weights(n, wk)
        times = _times(time, status, w, 7)
        assert times[-1] < time.max()
        got, ref = _check(gpu, _dev(X), eta, delta, cols, B, _hg(times, 3), times, time, status, w, "km",
                          "all censored w=%s" % wk)
        assert not got["row_a"].any() and (got["time_b"] >= 1.0).all() and got["time_b"][-1] > 100.0
        assert got["brier"][0].tolist() == [0.0, 0.0, 0.0]  # hg = 0 before the first baseline time, and a = 0


def test_times_below_the_smallest_row_time_and_at_the_largest_admissible_time(gpu):
    X, cols, B, time, status, eta, delta = _common()
    t = _dev(X)
    w = _weights(time.size, "eighths")
    below = np.array([0.25, 0.5, 0.999]) * time.min()
    hg = np.column_stack([[0.0, 0.5, 2.0]] * 3) * np.array([1.0, 1.5, 2.0])[None, :]  # (no row has left: b q^2 alone)
    got, _ = _check(gpu, t, eta, delta, cols, B, hg, below, time, status, w, "km", "below every row time")
    assert (got["time_b"] == 1.0).all() and got["brier"][0].tolist() == [0.0, 0.0, 0.0] and (got["brier"][1:] > 0).all()
    for st, what in ((status, "as drawn"), (np.where(time == time.max(), 0.0, status), "last row censored"),
                     (np.where(time == time.max(), 1.0, status), "last row an event")):
        last = _last_admissible(time, st, w)
        assert (last < time.max()) == (st[np.argmax(time)] == 0)
        times = np.array([np.median(time), last])
        got, _ = _check(gpu, t, eta, delta, cols, B, _hg(times, 3), times, time, st, w, "km",
                        "at the largest admissible time, " + what)
        if last < time.max():
            with pytest.raises(ValueError, match="largest admissible time"):
                gpu.cox_brier_device(t, cols, B, _hg(times, 3), np.array([times[0], time.max()]), time, st, weight=w)


def test_heavy_ties_with_row_times_equal_to_the_requested_times(gpu):
    X, cols, B, time, status, eta, delta = _common()
    tied = np.round(time, 1) + 0.1  # about 60 distinct values for 1025 rows
    u = np.unique(tied)
    assert u.size < 80
    for wk in ("none", "zeros"):
        w = _weights(tied.size, wk)
        times = u[u <= _last_admissible(tied, status, w)][::3]  # every requested time IS a row time (inclusive: it has left)
        assert np.isin(times, tied).all() and times.size >= 10
        _check(gpu, _dev(X), eta, delta, cols, B, _hg(times, 3), times, tied, status, w, "km", "ties w=%s" % wk)


def test_a_zero_hazard_gives_the_weighted_fraction_that_has_left(gpu):
    X, cols, B, time, status, eta, delta = _common()
    n, t = time.size, _dev(X)
    times = _times(time, status, None, 7)
    zero = np.zeros((7, 3))
    got, _ = _check(gpu, t, eta, delta, cols, B, zero, times, time, status, None, None, "hg = 0, unweighted")
    for j, tj in enumerate(times):  # sums of ones: exact, so the score is the count over n rounded once
        assert got["brier"][j].tolist() == [float(np.sum(status[time <= tj])) / n] * 3
    w = _weights(n, "zeros")
    got, ref = _check(gpu, t, eta, delta, cols, B, zero, times, time, status, w, "km", "hg = 0, km weights")
    want = np.array([(w.astype(LD) * got["row_a"].astype(LD))[time <= tj].sum() for tj in times]) / w.astype(LD).sum()
    assert (np.abs(ref["value"][:, 0] - want) <= LD(n) * LD(2.0) ** -63 * want).all()  # (longdouble sums in two orders)
    assert (np.abs(got["brier"].astype(LD) - want[:, None]) <= LD(n) * U * want[:, None]).all()


def test_a_survival_that_underflows_to_zero(gpu):
    X, cols, B, time, status, eta, delta = _common()
    w = _weights(time.size, "eighths")
    times = _times(time, status, w, 4)
    hg = np.column_stack([[1e6, 1e6, 1e6, 1e6], [300.0, 300.0, 300.0, 300.0], [0.0, 30.0, 300.0, 3000.0]])
    z = np.exp(np.asarray(eta[:, 1], dtype=np.float64)) * 300.0
    assert (z > 760).any() and (z < 700).any() and ((z > 708) & (z < 745)).any()  # (into and through the subnormals)
    got, ref = _check(gpu, _dev(X), eta, delta, cols, B, hg, times, time, status, w, "km", "S underflows")
    # model 0: S = 0 and q = 1 for every row, so the score is b times the weight still at risk, over W
    want = got["time_b"] * np.array([w[time > tj].sum() for tj in times]) / w.sum()
    assert (np.abs(got["brier"][:, 0] - want) <= 4 * float(U) * want).all()


# ----------------------------------------------------------------------------------------------------------------
# the C ABI, the estimator, a path
# ----------------------------------------------------------------------------------------------------------------
def test_c_abi_pointer_checks_ledger_and_bench(gpu):
    X, cols, B, time, status, eta, delta = _common()
    n, T, R = time.size, 3, 3
    t = _dev(X)
    times = _times(time, status, None, T)
    hg = np.ascontiguousarray(_hg(times, R).T)  # model-major
    row_a, time_b = gpu.ipcw_weights(time, status, times)
    lib = gpu.lib()
    before = gpu.process_counters()
    a = gpu.CoxBrierInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = X.ctypes.data, 0, P, 1, n, P  # x: a host pointer
    a.cols, a.m, a.B, a.R = gpu._ip(cols), 3, gpu._dp(B), R
    a.hg, a.times, a.T = gpu._dp(hg), gpu._dp(times), T
    a.time, a.row_a, a.time_b = gpu._dp(time), gpu._dp(row_a), gpu._dp(time_b)
    bs, sw = np.full((T, R), -7.0), ctypes.c_double(-7.0)
    assert lib.bessx_cox_brier_device(ctypes.byref(a), gpu._dp(bs), ctypes.byref(sw)) == 1 and b"x" in lib.bessx_last_error()
    assert (bs == -7.0).all() and sw.value == -7.0
    a.x, a.x_row_stride = t.data_ptr(), 1 << 24  # a view that reaches past its allocation
    assert lib.bessx_cox_brier_device(ctypes.byref(a), gpu._dp(bs), ctypes.byref(sw)) == 1
    a.x_row_stride = P
    assert lib.bessx_cox_brier_device(ctypes.byref(a), gpu._dp(bs), ctypes.byref(sw)) == 0, gpu.last_error()
    assert sw.value == float(n)
    ref = coxbrierref.brier_reference(eta, delta, hg.T, times, time, None, row_a, time_b, coxbrierref.device_depth(n, T))
    coxbrierref.check_brier(bs, ref, "C ABI")
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
    assert after["allocation_requests"] > before["allocation_requests"]
    for R_, T_ in ((1, 5), (3, 300)):
        ms = gpu.op_cox_brier_bench(t, cols, R=R_, T=T_, repeats=2)
        assert len(ms) == 3 and all(v > 0 for v in ms)
    assert gpu.process_counters()["live_device_bytes"] == before["live_device_bytes"]


def test_the_estimator_agrees_with_the_capi_route(gpu):
    X, obs, status, _, _ = synth.make_cox(300, 20, 3, seed=76)
    y = np.column_stack([obs, status])
    Xd = _dev(X)
    est = linear.PdasCox(sequence=[1, 2, 3, 4])
    est.fit(Xd, y)
    times = np.quantile(obs, [0.05, 0.2, 0.4, 0.6, 0.8])
    with pytest.raises(ValueError, match="fit_baseline"):
        est.brier_survival(Xd, y, times)
    cols = np.nonzero(est.beta)[0]
    assert cols.size > 0
    B = est.beta[cols].reshape(-1, 1)
    eta, delta = evalref.eta_reference(X, cols, B, [0.0])
    w = np.random.default_rng(7).integers(1, 17, 300) / 8.0
    for wt in (None, w):
        est.fit_baseline(Xd, _dev(y), weight=None if wt is None else _dev(wt))
        hg = gpu.baseline_at(est.baseline_times_, est.baseline_cumhaz_, times).reshape(-1, 1)
        got = est.brier_survival(Xd, _dev(y), times, weight=None if wt is None else _dev(wt))
        direct = gpu.cox_brier_device(Xd, cols, B, hg, times, obs, status, weight=wt)
        assert got["brier"].shape == (5,) and got["ipa"].shape == (5,) and isinstance(got["ibs"], float)
        for k in ("brier", "ipa"):
            assert np.array_equal(_bits(got[k]), _bits(direct[k][:, 0])), k
        for k in ("null", "row_a", "time_b"):
            assert np.array_equal(_bits(got[k]), _bits(direct[k])), k
        assert got["ibs"] == direct["ibs"][0] and got["ibs_null"] == direct["ibs_null"] and got["sum_w"] == direct["sum_w"]
        ref = coxbrierref.brier_reference(eta, delta, hg, times, obs, wt, got["row_a"], got["time_b"],
                                          coxbrierref.device_depth(300, 5), "estimator")
        coxbrierref.check_brier(got["brier"].reshape(-1, 1), ref, "estimator, device")
        host = linear.PdasCox()
        host.p, host.beta, host.coef0 = est.p, est.beta, est.coef0
        host.baseline_times_, host.baseline_cumhaz_ = est.baseline_times_, est.baseline_cumhaz_
        other = host.brier_survival(X, y, times, weight=wt)  # the NumPy route from the same baseline: the same reference
        coxbrierref.check_brier(other["brier"].reshape(-1, 1), ref, "estimator, numpy")
        assert 0.0 < got["ibs"] < got["ibs_null"]  # a fitted model beats the Kaplan-Meier curve on its own rows


def test_candidates_of_a_cox_path_are_chosen_by_integrated_brier_score_on_held_out_rows(gpu):
    X, obs, status, _, _ = synth.make_cox(700, 30, 3, seed=76)  # (rows in time order, as the session wants them)
    pick = np.random.default_rng(2).permutation(700)
    tr, va = np.sort(pick[:400]), np.sort(pick[400:])
    with gpu.Session(X[tr], status[tr], data_type=3, model_type=4) as s:
        result = s.sequential_path(np.arange(1, 6), ic_type=3)
    R = len(result["cand_coef0"])
    assert R == 5
    Xt, Xv = _dev(X[tr]), _dev(X[va])
    times = np.quantile(obs[va], np.linspace(0.05, 0.8, 16))
    ibs, best = gpu.cox_brier_candidates(result, Xt, obs[tr], status[tr], Xv, obs[va], status[va], times)
    assert isinstance(ibs, np.ndarray) and ibs.shape == (R,) and isinstance(best, int)
    a, b = gpu.ipcw_weights(obs[va], status[va], times)
    coxbrierref.check_ipcw(a, b, coxbrierref.ipcw_reference(obs[va], status[va], times, None), 300, "candidates")
    want, bound = np.zeros(R, dtype=LD), np.zeros(R, dtype=LD)
    dt = np.diff(times).astype(LD)
    for r in range(R):
        sup = result["cand_support"][r]
        sup = sup[sup >= 0]
        order = np.argsort(sup)
        c, beta = sup[order], result["cand_beta"][r][:sup.size][order]
        base = gpu.cox_baseline_device(Xt, c, beta, obs[tr], status[tr])  # (checked by tests/test_cox_surv_gpu.py)
        hg = gpu.baseline_at(base["times"], base["cumhaz"], times).reshape(-1, 1)
        eta, delta = evalref.eta_reference(X[va], c, beta.reshape(-1, 1), [0.0])
        ref = coxbrierref.brier_reference(eta, delta, hg, times, obs[va], None, a, b, coxbrierref.device_depth(300, 16),
                                          "candidate %d" % r)
        span = LD(times[-1]) - LD(times[0])
        trap = lambda v: (LD(0.5) * dt * (v[1:, 0] + v[:-1, 0])).sum() / span
        want[r] = trap(ref["value"])
        bound[r] = trap(ref["bound"]) + evalref.gamma(3 * 16 + 4) * want[r]  # the trapezoid rule's own roundings
        print("candidate %d: IBS %.12e, err %.3e against bound %.3e" % (r, ibs[r], float(abs(LD(ibs[r]) - want[r])),
                                                                         float(bound[r])))
        assert abs(LD(ibs[r]) - want[r]) <= bound[r]
    two = np.sort(want)[:2]
    assert two[1] - two[0] > 100 * bound.max(), "the two best candidates are too close for this seed"
    assert best == int(np.argmin(want))
