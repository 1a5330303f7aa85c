"""Held-out Cox partial log-likelihood and concordance on an X already in GPU memory (bessx_eval_cox_device,
bess_amd/csrc/bessx_k_coxeval.hip) against NumPy in np.longdouble on the host copy of the same values.  The bound is
derived in tests/coxevalref.py; the pair counts are compared exactly after coxevalref.count_precondition has held on
every comparable pair of every case.  Where two routes are compared with each other each is within its bound of the
exact value, so they agree within the sum of the bounds.  The one tolerance that is not derived is that of train_loss
(rtol 1e-7, atol 1e-9), taken from tests/test_golden_gpu.py."""
import ctypes

import numpy as np
import pytest

import coxevalref
import evalref
from bess_amd import linear, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
_DATA, _REFS = {}, {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _data(n_full, p, seed, dtype=np.float64):
    """make_cox rows in a shuffled order (so that a row's position is not its number), as values of `dtype`."""
    key = (n_full, p, seed, np.dtype(dtype).name)
    if key not in _DATA:
        X, obs, status, _, _ = synth.make_cox(n_full, p, 3, seed=seed)
        perm = np.random.default_rng(seed).permutation(n_full)
        _DATA[key] = (np.ascontiguousarray(X[perm]).astype(dtype), obs[perm].copy(), status[perm].copy())
    return _DATA[key]


def _model(p, m, R, seed, share=0.3):
    """The union of the supports (m ascending columns) and B (m, R): N(0, 0.25) coefficients; with R > 1 every model
    leaves out about `share` of the union but keeps at least one column."""
    rng = np.random.default_rng(1000 + seed + 10 * R)
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    B = rng.normal(0.0, 0.5, (m, R))
    if R > 1:
        drop = rng.uniform(size=(m, R)) < share
        drop[rng.integers(0, m, R), np.arange(R)] = False
        B[drop] = 0.0
    return cols, B


def _ref(key, vals, cols, B, time, status, w, ties, counts=True):
    """(loglik reference, exact counts or None), computed once per key; the precondition of the counts is asserted."""
    if key not in _REFS:
        eta, delta = evalref.eta_reference(vals, cols, B, np.zeros(B.shape[1]))
        cnt = None
        if counts:
            gap = coxevalref.count_precondition(vals, cols, B, eta, delta, time, status, str(key))
            print("%s: smallest gap / required gap %.3e" % (key, gap))
            cnt = coxevalref.pair_counts(eta, time, status)
        _REFS[key] = (eta, delta, cnt)
    eta, delta, cnt = _REFS[key]
    return coxevalref.loglik_reference(eta, delta, time, status, w, ties), cnt


def _check(got, ref, cnt, what):
    coxevalref.check_loglik(got["loglik"], ref, what)
    coxevalref.check_counts(got, cnt, what)
    num = got["concordant"].astype(np.float64) + 0.5 * got["tied_risk"].astype(np.float64)
    if cnt["comparable"] > 0:
        assert np.array_equal(got["c_index"], num / cnt["comparable"]), what
    else:
        assert np.isnan(got["c_index"]).all(), what


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_scan_and_tile_edges(gpu, n):
    X, time, status = _data(2049, 24, 81)
    X, time, status = X[:n], time[:n], status[:n].copy()
    if n <= 2:
        status[0] = 1.0  # (an event, so that the likelihood has a term)
    cols, B = _model(24, 5, 1, 81)
    for ties in ("order", "breslow"):
        ref, cnt = _ref(("edges", n), X, cols, B, time, status, None, ties)
        got = gpu.evaluate_cox_device(_dev(X), cols, B, time, status, ties=ties)
        assert got["loglik"].shape == (1,) and got["concordant"].dtype == np.int64
        _check(got, ref, cnt, "n=%d %s" % (n, ties))
        again = gpu.evaluate_cox_device(_dev(X), cols, B, time, status, ties=ties, concordance=False)
        assert set(again) == {"loglik", "comparable"} and again["comparable"] == cnt["comparable"]
        assert np.array_equal(_bits(again["loglik"]), _bits(got["loglik"]))


def test_no_event_is_not_an_error(gpu):
    X, time, status = _data(2049, 24, 81)
    X, time = X[:300], time[:300]
    cols, B = _model(24, 5, 1, 81)
    none = np.zeros(300)
    ref, cnt = _ref(("no event",), X, cols, B, time, none, None, "order")
    assert ref["loglik"][0] == 0 and ref["bound"][0] == 0 and cnt["comparable"] == 0
    got = gpu.evaluate_cox_device(_dev(X), cols, B, time, none)
    _check(got, ref, cnt, "no event")
    assert got["comparable"] == 0 and np.isnan(got["c_index"]).all()


@pytest.mark.parametrize("R", [1, 3, 5, 9])
def test_r_tiles_with_a_union_of_supports(gpu, R):
    n = 1025
    X, time, status = _data(1025, 24, 83)
    cols, B = _model(24, 9, R, 83)
    w = np.random.default_rng(5).integers(1, 17, n) / 8.0
    t = _dev(X)
    for ties in ("order", "breslow"):
        ref, cnt = _ref(("tiles", R), X, cols, B, time, status, w, ties)
        got = gpu.evaluate_cox_device(t, cols, B, time, status, weight=w, ties=ties)
        _check(got, ref, cnt, "R=%d %s" % (R, ties))
        again = gpu.evaluate_cox_device(t, cols, B, time, status, weight=w, ties=ties)
        for k in got:
            assert np.array_equal(np.asarray(got[k]).view(np.int64), np.asarray(again[k]).view(np.int64)), k
    clean = gpu.evaluate_cox_device(t, cols, B, time, status, weight=w)
    ref, cnt = _ref(("tiles", R), X, cols, B, time, status, w, "order")
    if R == 5:  # every model alone, in the same tile arrangement (the other four columns of B zero)
        for r in range(R):
            alone = np.zeros_like(B)
            alone[:, r] = B[:, r]
            one = gpu.evaluate_cox_device(t, cols, alone, time, status, weight=w)
            assert _bits(one["loglik"])[r] == _bits(clean["loglik"])[r], r
            for k in ("concordant", "discordant", "tied_risk"):
                assert one[k][r] == clean[k][r], (k, r)
    # a NaN in one support column reaches exactly the models that use it
    k = int(np.argmax((B != 0).sum(axis=1) < R)) if R > 1 else 0
    uses = B[k] != 0.0
    assert uses.any() and (R == 1 or not uses.all())
    bad = X.copy()
    bad[321, cols[k]] = np.nan
    got = gpu.evaluate_cox_device(_dev(bad), cols, B, time, status, weight=w)
    assert np.array_equal(np.isnan(got["loglik"]), uses)
    assert coxevalref.within(got["loglik"], ref)[~uses].all()
    assert np.array_equal(_bits(got["loglik"])[~uses], _bits(clean["loglik"])[~uses])
    for name in ("concordant", "discordant", "tied_risk"):
        assert np.array_equal(got[name][~uses], cnt[name][~uses]), name


def _views(vals):
    """name -> (base host array with NaN outside the view, base tensor -> the n x p view)"""
    n, p = vals.shape
    F = np.full((p, (n + 3) // 4 * 4), np.nan)
    F[:, :n] = vals.T
    S = np.full((2 * n, p + 1), np.nan)
    S[::2, 1:] = vals
    P = np.full((n, p + 7), np.nan)
    P[:, :p] = vals
    return {"f64 row-major": (vals.copy(), lambda t: t), "f64 column-major": (F, lambda t: t[:, :n].T),
            "f32 row-major": (vals.astype(np.float32), lambda t: t), "strided slice": (S, lambda t: t[::2, 1:]),
            "padded rows": (P, lambda t: t[:, :p])}


@pytest.mark.parametrize("view", ["f64 row-major", "f64 column-major", "f32 row-major", "strided slice", "padded rows"])
def test_views_of_x(gpu, view):
    n = 513
    X, time, status = _data(513, 16, 84)
    base, take = _views(X)[view]
    vals = base.astype(np.float64) if view == "f32 row-major" else X  # (the widened values)
    cols, B = _model(16, 3, 3, 84, share=0.0)
    t = take(_dev(base))
    assert tuple(t.shape) == (n, 16)
    for ties in ("order", "breslow"):
        ref, cnt = _ref(("views", view == "f32 row-major"), vals, cols, B, time, status, None, ties)
        _check(gpu.evaluate_cox_device(t, cols, B, time, status, ties=ties), ref, cnt, "%s %s" % (view, ties))


def test_the_clamp_keeps_large_predictors_finite_and_inside_the_bound(gpu):
    X, time, status = _data(513, 16, 84)
    cols, B = _model(16, 3, 3, 84, share=0.0)
    B = B * np.array([1.0, 40.0, 150.0])[None, :]
    eta, _ = evalref.eta_reference(X, cols, B, np.zeros(3))
    assert (np.abs(eta[:, 1:]) > 30).any(axis=0).all() and (eta[:, 2] > 30).any() and (eta[:, 2] < -30).any()
    for ties in ("order", "breslow"):
        ref, cnt = _ref(("clamp",), X, cols, B, time, status, None, ties)
        got = gpu.evaluate_cox_device(_dev(X), cols, B, time, status, ties=ties)
        assert np.isfinite(got["loglik"]).all()
        _check(got, ref, cnt, "clamp " + ties)


_ABSORB_AT = (4, 252, 256, 260, 1028)  # first scan index of the thread that holds the large term, one model each


def _absorbing_case():
    """The pattern at which a scan that forms a thread's exclusive offset as inclusive - own total loses everything: in
    scan order (from the latest time down; a thread of k_cxe_scan_apply owns scan indices 4 t .. 4 t + 3 of its block of
    1024) every term before scan index j0 + 3 is exp(-30) and the term at j0 + 3, the last of the SAME thread, is
    exp(+30).  The thread's own total then absorbs the running sum in front of it (e^60 > 2^53), while S at its first
    three elements is still a handful of e^-30 and has to come out to full relative accuracy.  One model per j0 in
    _ABSORB_AT: lane 1 and lane 63 of the first wave, lanes 0 and 1 of the second wave (the offset of the waves before),
    and lane 1 of the second block (the carry of the blocks before).  Model 5 is a staircase in one thread chain, where
    the loss would be partial: e^-30 up to index 6, e^0 from 7 to 10, e^30 at 11, i.e. thread 2 holds 1, 1, 1, e^30
    behind a running sum of about 1.  Model r reads column r alone (B is diagonal, coefficient 1), so eta is x itself:
    -40 and +40 are clamped, the rest is N(0, 9).  Every row is an event, times are distinct and shuffled against the
    row numbers.  Rows that share a value of x are identical on the model's support: exact ties for the counts."""
    n, R = 1040, len(_ABSORB_AT) + 1
    rng = np.random.default_rng(85)
    scan = 3.0 * rng.standard_normal((n, R))  # by scan index
    for r, j0 in enumerate(_ABSORB_AT):
        scan[:j0 + 3, r] = -40.0
        scan[j0 + 3, r] = 40.0
    scan[:7, R - 1], scan[7:11, R - 1], scan[11, R - 1] = -40.0, 0.0, 40.0
    rows = rng.permutation(n)  # rows[k]: the row at position k
    X = np.empty((n, R))
    X[rows] = scan[::-1]
    time = np.empty(n)
    time[rows] = 0.5 + np.arange(n)
    return X, time, np.ones(n), np.arange(R, dtype=np.int32), np.eye(R)


def test_the_scan_keeps_small_risk_sets_behind_a_large_term_of_the_same_thread(gpu):
    X, time, status, cols, B = _absorbing_case()
    order = np.argsort(time, kind="stable")
    for r, j0 in enumerate(_ABSORB_AT):  # (the case is what its docstring says, in positions)
        assert (X[order[::-1][:j0 + 3], r] == -40.0).all() and X[order[::-1][j0 + 3], r] == 40.0
    for ties in ("order", "breslow"):
        ref, cnt = _ref(("absorb",), X, cols, B, time, status, None, ties)
        _check(gpu.evaluate_cox_device(_dev(X), cols, B, time, status, ties=ties), ref, cnt, "absorbing " + ties)


def _tied_case():
    """600 rows, times rounded to 2 decimals (many tie groups), rows 100..149 duplicates of rows 0..49 with their own
    times and status (exact ties of the risk between comparable rows)."""
    X, time, status = _data(2049, 24, 81)
    X, time, status = X[:600].copy(), np.round(time[:600], 2), status[:600]
    X[100:150] = X[:50]
    return X, time, status


def test_tied_times_and_duplicated_rows(gpu):
    X, time, status = _tied_case()
    assert np.unique(time).size < 300
    cols, B = _model(24, 5, 3, 81)
    w = np.random.default_rng(6).integers(1, 17, 600) / 8.0
    out = {}
    for ties in ("order", "breslow"):
        ref, cnt = _ref(("ties",), X, cols, B, time, status, w, ties)
        out[ties] = gpu.evaluate_cox_device(_dev(X), cols, B, time, status, weight=w, ties=ties)
        _check(out[ties], ref, cnt, "tied times " + ties)
    assert (out["order"]["tied_risk"] >= 1).all()


def test_device_vectors_give_the_result_of_host_vectors(gpu):
    X, time, status = _tied_case()
    cols, B = _model(24, 5, 3, 81)
    w = np.random.default_rng(6).integers(1, 17, 600) / 8.0
    t = _dev(X)
    want = gpu.evaluate_cox_device(t, cols, B, time, status, weight=w, ties="breslow")
    got = gpu.evaluate_cox_device(t, cols, B, _dev(time), _dev(status), weight=_dev(w), ties="breslow")
    t32 = time.astype(np.float32)
    want32 = gpu.evaluate_cox_device(t, cols, B, t32.astype(np.float64), status, weight=w, ties="breslow")
    got32 = gpu.evaluate_cox_device(t, cols, B, _dev(t32), _dev(status.astype(np.float32)),
                                    weight=_dev(w.astype(np.float32)), ties="breslow")
    for a, b in ((want, got), (want32, got32)):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)), k


def test_the_estimator_against_its_fit_and_against_the_numpy_route(gpu):
    X, obs, status, _, _ = synth.make_cox(1500, 40, 4, seed=76)
    y = np.column_stack([obs, status])
    est = linear.PdasCox(sequence=[1, 2, 3, 4, 5, 6])
    est.fit(_dev(X[:1000]), y[:1000])
    train = est.evaluate_survival(_dev(X[:1000]), y[:1000])
    train_loss = float(np.ravel(est.train_loss)[0])
    print("deviance %.12e, train_loss %.12e" % (train["deviance"], train_loss))
    assert np.isclose(train["deviance"], train_loss, rtol=1e-7, atol=1e-9)
    assert est.concordance(_dev(X[:1000]), y[:1000]) > 0.5
    assert est.evaluate(_dev(X[:1000]), y[:1000]) is None and est.predict(_dev(X[:1000])) is None
    Xv, yv = X[1000:], y[1000:]
    w = np.random.default_rng(7).integers(1, 17, 500) / 8.0
    cols = np.nonzero(est.beta)[0]
    B = est.beta[cols].reshape(-1, 1)
    for ties in ("order", "breslow"):
        for wt in (None, w):
            ref, cnt = _ref(("fit",), Xv, cols, B, yv[:, 0], yv[:, 1], wt, ties)
            dev = est.evaluate_survival(_dev(Xv), _dev(yv), weight=None if wt is None else _dev(wt), ties=ties)
            host = est.evaluate_survival(Xv, yv, weight=wt, ties=ties)
            assert set(dev) == set(host)
            assert all(type(dev[k]) is type(host[k]) and type(dev[k]) in (float, int) for k in dev)
            coxevalref.check_loglik([dev["loglik"]], ref, "device " + ties)
            coxevalref.check_loglik([host["loglik"]], ref, "numpy " + ties)
            assert abs(LD(dev["loglik"]) - LD(host["loglik"])) <= 2 * ref["bound"][0]
            coxevalref.check_counts(dev, cnt)
            coxevalref.check_counts(host, cnt)
            assert dev["c_index"] == host["c_index"] and dev["n_events"] == host["n_events"]
            assert dev["deviance"] == -2.0 * dev["loglik"]


@pytest.mark.parametrize("family", ["cox", "lm"])
def test_linear_predictor_on_a_device_x(gpu, family):
    if family == "cox":
        X, obs, status, _, _ = synth.make_cox(700, 30, 3, seed=77)
        est = linear.PdasCox(sequence=[1, 2, 3, 4])
        est.fit(_dev(X[:500]), np.column_stack([obs, status])[:500])
    else:
        X, y, _, _ = synth.make_lm(700, 30, 3, seed=78)
        est = linear.PdasLm(sequence=[1, 2, 3, 4])
        est.fit(_dev(X[:500]), y[:500])
    Xv = X[500:]
    cols = np.nonzero(est.beta)[0]
    assert cols.size > 0
    eta, delta = evalref.eta_reference(Xv, cols, est.beta[cols].reshape(-1, 1), [est.coef0])
    got = est.linear_predictor(_dev(Xv))
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (200,)
    err = np.abs(got.cpu().numpy().astype(LD) - eta[:, 0])
    print("%s: max err / Delta %.3e" % (family, float((err / delta[:, 0]).max())))
    assert (err <= delta[:, 0]).all()
    host = est.linear_predictor(Xv)
    assert isinstance(host, np.ndarray) and (np.abs(host.astype(LD) - eta[:, 0]) <= delta[:, 0]).all()


def test_candidates_of_a_cox_path_are_chosen_on_held_out_rows(gpu):
    X, obs, status, _, _ = synth.make_cox(1500, 40, 4, seed=76)
    with gpu.Session(X[:1000], status[:1000], data_type=3, model_type=4) as s:
        result = s.sequential_path(np.arange(1, 9), ic_type=3)
    R = len(result["cand_coef0"])
    assert R == 8
    Xv, tv, sv = X[1000:], obs[1000:], status[1000:]
    t = _dev(Xv)
    ll, best = gpu.evaluate_cox_candidates(result, t, tv, sv)
    assert isinstance(ll, np.ndarray) and ll.shape == (R,) and isinstance(best, int)
    want, bound = np.zeros(R, dtype=LD), np.zeros(R, dtype=LD)
    for r in range(R):
        sup = result["cand_support"][r]
        sup = sup[sup >= 0]
        order = np.argsort(sup)
        c, b = sup[order], result["cand_beta"][r][:sup.size][order].reshape(-1, 1)
        ref, _ = _ref(("cand", r), Xv, c, b, tv, sv, None, "order", counts=False)
        want[r], bound[r] = ref["loglik"][0], ref["bound"][0]
        one = gpu.evaluate_cox_device(t, c, b, tv, sv, concordance=False)["loglik"][0]
        assert abs(LD(one) - want[r]) <= bound[r]
        assert abs(LD(one) - LD(ll[r])) <= 2 * bound[r]
    err = np.abs(ll.astype(LD) - want)
    print("candidates: max err / bound %.3e" % float((err / bound).max()))
    assert (err <= bound).all()
    two = np.argsort(-want)[:2]
    assert want[two[0]] - want[two[1]] > bound[two[0]] + bound[two[1]], "choose another seed"
    assert best == int(two[0])


def test_c_abi_through_ctypes(gpu):
    X, time, status = _tied_case()
    cols, B = _model(24, 5, 3, 81)
    w = np.random.default_rng(6).integers(1, 17, 600) / 8.0
    t = _dev(X)
    Bc = np.ascontiguousarray(B)

    def call(weight, ties, want_pairs):
        a = gpu.CoxEvalInput()
        a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = t.data_ptr(), 0, 24, 1, 600, 24
        a.cols, a.m, a.B, a.R = gpu._ip(cols), 5, gpu._dp(Bc), 3
        a.time, a.status, a.weight = gpu._dp(time), gpu._dp(status), gpu._dp(weight)
        a.ties, a.want_pairs = ties, want_pairs
        ll, pairs, comp = np.full(3, -7.0), np.full((3, 3), -7, dtype=np.int64), ctypes.c_longlong(-7)
        pp = pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)) if want_pairs else None
        rc = gpu.lib().bessx_eval_cox_device(ctypes.byref(a), gpu._dp(ll), pp, ctypes.byref(comp))
        assert rc == 0, gpu.last_error()
        return ll, pairs, comp.value

    before = gpu.process_counters()
    for weight in (w, None):
        for ties in (0, 1):
            name = "breslow" if ties else "order"
            ref, cnt = _ref(("ties",), X, cols, B, time, status, weight, name)
            ll, pairs, comp = call(weight, ties, 1)
            coxevalref.check_loglik(ll, ref, "C ABI %s" % name)
            assert comp == cnt["comparable"]
            for j, k in enumerate(("concordant", "discordant", "tied_risk")):
                assert np.array_equal(pairs[:, j], cnt[k]), k
            ll0, pairs0, comp0 = call(weight, ties, 0)
            assert np.array_equal(_bits(ll0), _bits(ll)) and comp0 == comp and (pairs0 == -7).all()
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["allocation_requests"] > before["allocation_requests"]
    ms = gpu.op_cox_eval_bench(t, cols, R=3, ties="breslow", repeats=2)
    assert len(ms) == 3 and all(v > 0 for v in ms)
    assert gpu.op_cox_eval_bench(t, cols, R=3, concordance=False, repeats=2)[2] == 0.0
    assert gpu.process_counters()["live_device_bytes"] == before["live_device_bytes"]
