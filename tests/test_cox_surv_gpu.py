"""Breslow baseline hazard and survival curves on an X already in GPU memory (bessx_cox_baseline_device,
bessx_cox_survival_device, bess_amd/csrc/bessx_k_coxsurv.hip) against NumPy in np.longdouble on the host copy of the same
values.  The bounds are derived in tests/coxsurvref.py; every check prints error against bound, and every case that is not
marked adversarial also asserts that the bound itself is at most 1e-9.  The shapes are the smallest that reach every path:
the 1024-position scan blocks, the 128 / 256-row predictor workgroups, both branches of the predictor's chunk loop and
both lane groupings of its gather kernel, the 256-row and 512-row tiles of the curve kernels, their 16-byte and element
stores, and the 64-column chunks of hg."""
import ctypes

import numpy as np
import pytest

import coxsurvref
import evalref
from bess_amd import linear, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
P = 80
_REFS = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _problem(n, m, seed=91):
    """X (n x P, N(0, 1)), m ascending support columns with coefficients N(0, 1 / m) (|eta| stays below 5), continuous
    times in an order that is not the rows', about 60% events."""
    rng = np.random.default_rng(seed + 7 * m)
    X = rng.standard_normal((4099, P))[:n]
    cols = np.sort(rng.choice(P, m, replace=False)).astype(np.int32)
    B = rng.standard_normal(m) / np.sqrt(max(m, 1))
    time = rng.exponential(1.0, 4099)[:n]
    status = (rng.uniform(size=4099) < 0.6).astype(np.float64)[:n]
    return X, cols, B, time, status


def _weights(n, kind):
    if kind == "none":
        return None
    w = np.random.default_rng(5).integers(1, 17, 4099)[:n] / 8.0
    if kind == "zeros":
        w[::3] = 0.0
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
        eta, delta = evalref.eta_reference(vals, cols, np.asarray(B).reshape(-1, 1), [0.0])
        _REFS[key] = (eta[:, 0], delta[:, 0])
    return _REFS[key]


# ----------------------------------------------------------------------------------------------------------------
# the baseline
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 4099])
def test_baseline_at_the_block_edges_for_every_layout_and_support(gpu, n):
    for m in (0, 1, 3, 70):
        X, cols, B, time, status = _problem(n, m)
        if n <= 2:
            status = np.ones(n)
        for layout in LAYOUTS:
            t, vals = _view(X, layout)
            assert tuple(t.shape) == (n, P)
            eta, delta = _eta(("edges", n, m, layout == "f32 row-major"), vals, cols, B)
            for wk in (("none", "random", "zeros") if layout == "f64 row-major" else ("none",)):
                w = _weights(n, wk)
                ref = coxsurvref.baseline_reference(eta, delta, time, status, w)
                got = gpu.cox_baseline_device(t, cols, B, time, status, weight=w)
                assert set(got) == {"times", "cumhaz", "n_events"}
                coxsurvref.check_baseline(got["times"], got["cumhaz"], ref, "n=%d m=%d %s w=%s" % (n, m, layout, wk))
                assert got["n_events"] == float(np.sum(status if w is None else w * status))
        again = gpu.cox_baseline_device(t, cols, B, time, status)
        assert np.array_equal(_bits(again["cumhaz"]), _bits(got["cumhaz"]))


def test_baseline_with_a_tie_group_across_a_block_boundary_and_the_status_patterns(gpu):
    n, m = 2049, 3
    X, cols, B, _, status = _problem(n, m)
    rows = np.random.default_rng(3).permutation(n)  # rows[k]: the row at position k
    tpos = np.arange(n, dtype=np.float64)
    tpos[1020:1031] = 1020.0  # one tie group over positions 1020..1030
    time = np.empty(n)
    time[rows] = tpos
    eta, delta = _eta(("ties",), X, cols, B)
    t = _dev(X)
    last = np.zeros(n)
    last[rows[-1]] = 1.0
    group_censored = status.copy()
    group_censored[rows[1020:1031]] = 0.0
    for what, st in (("random status", status), ("all events", np.ones(n)), ("event at the last position only", last),
                     ("tie group censored", group_censored)):
        ref = coxsurvref.baseline_reference(eta, delta, time, st, None)
        got = gpu.cox_baseline_device(t, cols, B, time, st)
        coxsurvref.check_baseline(got["times"], got["cumhaz"], ref, what)
        assert (1020.0 in got["times"]) == (what in ("random status", "all events")), what
    assert gpu.cox_baseline_device(t, cols, B, time, last)["times"].tolist() == [float(n - 1)]
    none = gpu.cox_baseline_device(t, cols, B, time, np.zeros(n), weight=_weights(n, "random"))
    assert none["times"].shape == (0,) and none["cumhaz"].shape == (0,) and none["n_events"] == 0.0  # J = 0


@pytest.mark.parametrize("j0", [4, 252, 1028])
def test_a_risk_set_of_small_terms_behind_a_large_one_keeps_its_hazard(gpu, j0):
    """Absorption in S, the construction of tests/test_cox_eval_gpu.py: in scan order (from the latest time down) every
    term before scan index j0 + 3 is exp(-30) and the term at j0 + 3, the last of the same thread, is exp(+30).  The
    hazard terms 1 / S of the positions behind it are about e^30 / j and have to come out to full relative accuracy."""
    n = 1040
    scan = np.full(n, -40.0)
    scan[j0 + 3] = 40.0
    scan[j0 + 4:] = 3.0 * np.random.default_rng(85).standard_normal(n - j0 - 4)
    rows = np.random.default_rng(86).permutation(n)
    X = np.zeros((n, 2))
    X[rows, 1] = scan[::-1]
    time = np.empty(n)
    time[rows] = 0.5 + np.arange(n)
    cols, B = np.array([1], dtype=np.int32), np.array([1.0])
    eta, delta = evalref.eta_reference(X, cols, B.reshape(1, 1), [0.0])
    ref = coxsurvref.baseline_reference(eta, delta, time, np.ones(n), None)
    got = gpu.cox_baseline_device(_dev(X), cols, B, time, np.ones(n))
    coxsurvref.check_baseline(got["times"], got["cumhaz"], ref, "absorbing S, j0=%d" % j0, ordinary=False)


@pytest.mark.parametrize("at", [9, 261, 1029])
def test_the_prefix_keeps_small_sums_in_front_of_a_weight_of_2_to_the_80(gpu, at):
    """Absorption in H: every row is an event of weight 1 except the one at position `at`, the second of its thread's four
    consecutive positions (4 t .. 4 t + 3 of a 1024-position block), whose weight is 2^80.  An exclusive offset formed as
    inclusive - own total gives 0 or noise for that thread, so H at position `at` - 1 (and at the groups before it in the
    same thread) would be lost; with additions only it is exact to its own size, and the groups after the large term are
    inside the bound too."""
    n = 2049
    assert at % 4 == 1
    rows = np.random.default_rng(87).permutation(n)
    X = np.random.default_rng(88).standard_normal((n, 4))
    time = np.empty(n)
    time[rows] = 1.0 + np.arange(n)
    w = np.ones(n)
    w[rows[at]] = 2.0 ** 80
    cols, B = np.array([], dtype=np.int32), np.array([])
    ref = coxsurvref.baseline_reference(np.zeros(n), np.zeros(n), time, np.ones(n), w)
    got = gpu.cox_baseline_device(_dev(X), cols, B, time, np.ones(n), weight=w)
    coxsurvref.check_baseline(got["times"], got["cumhaz"], ref, "weight 2^80 at position %d" % at, ordinary=False)
    before = slice(0, at)  # the groups BEFORE the large term, on their own: the bound there knows nothing of 2^80
    assert float(ref["bound"][before].max()) < 1e-12 and float(ref["cumhaz"][at]) > 2.0 ** 68
    assert (np.abs(got["cumhaz"][before].astype(LD) - ref["cumhaz"][before]) <= ref["bound"][before]).all()


# ----------------------------------------------------------------------------------------------------------------
# the curves
# ----------------------------------------------------------------------------------------------------------------
N_CURVES, M_CURVES = 1025, 5
_BT = np.cumsum(np.random.default_rng(11).uniform(0.01, 0.2, 40))
_BH = np.cumsum(np.random.default_rng(12).uniform(0.0, 0.1, 40))


def _grid(T):
    """T times before the first baseline time, at, between and after the baseline times, unsorted and repeated (as far
    as T entries hold them)."""
    must = [_BT[0] - 0.5, _BT[7], 0.5 * (_BT[3] + _BT[4]), _BT[-1] + 1.0, _BT[7], _BT[0], _BT[0] - 0.25]
    if T == 1:
        return np.array([_BT[7]])
    rng = np.random.default_rng(T)
    g = np.concatenate([must, rng.uniform(_BT[0] - 0.1, _BT[-1] + 0.1, max(T - len(must), 0))])[:T]
    return g[rng.permutation(T)]


def _curves_case():
    if "curves" not in _REFS:
        X, cols, B, _, _ = _problem(N_CURVES, M_CURVES)
        _REFS["curves"] = (X, cols, B) + _eta(("curves-eta",), X, cols, B)
    return _REFS["curves"]


def _out(variant, n, T):
    """(buffer filled with -7, the n x T view of it to write into, or None for a host result)"""
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")
    if variant == "host":
        return None, None
    if variant == "row-major":
        b = f(n, T)
        return b, b
    if variant == "column-major":  # column stride n = 1025, odd: element stores
        b = f(T, n)
        return b, b.T
    if variant == "column-major, even stride":  # 16-byte stores along the rows
        b = f(T, n + 1)
        return b, b[:, :n].T
    if variant == "padded rows":  # row stride T + 3: even for odd T (16-byte stores), odd for even T (element stores)
        b = f(n, T + 3)
        return b, b[:, :T]
    if variant == "offset by one":  # a base that is not 16-byte aligned
        b = f(n * T + 1)
        return b, b[1:].view(n, T)
    b = f(n, 2 * T)  # both strides > 1
    return b, b[:, ::2]


OUTS = ["row-major", "column-major", "column-major, even stride", "padded rows", "offset by one", "strided", "host"]


@pytest.mark.parametrize("T", [1, 2, 3, 63, 64, 65, 257])
def test_curves_for_every_chunk_edge_kind_and_layout_of_out(gpu, T):
    X, cols, B, eta, delta = _curves_case()
    n, t, grid = N_CURVES, _dev(X), _grid(T)
    hg = gpu.baseline_at(_BT, _BH, grid)
    assert T == 1 or (hg == 0.0).any()

    class Plain:  # a device array that is not a torch tensor: the result is a host array
        __cuda_array_interface__ = t.__cuda_array_interface__

    plain = Plain()
    before = gpu.process_counters()
    for kind in ("survival", "cumhaz"):
        ref = coxsurvref.curve_reference(eta, delta, hg, kind)
        first = None
        for variant in OUTS:
            buf, view = _out(variant, n, T)
            got = gpu.cox_survival_device(t, cols, B, _BT, _BH, times=grid, kind=kind, out=view)
            if variant == "host":
                assert isinstance(got, torch.Tensor) and got.is_cuda  # (a torch X: the result is allocated on its device)
                got = gpu.cox_survival_device(plain, cols, B, _BT, _BH, times=grid, kind=kind)
                assert isinstance(got, np.ndarray) and got.shape == (n, T)
                res = got
            else:
                assert got is view
                res = view.cpu().numpy()
                view.fill_(-7.0)  # the bytes outside the view are untouched: with the view reset, all is the sentinel
                assert bool((buf == -7.0).all()), variant
            coxsurvref.check_curves(res, ref, "T=%d %s %s" % (T, kind, variant))
            assert (res[:, hg == 0.0] == (1.0 if kind == "survival" else 0.0)).all()
            if first is None:
                first = _bits(res)
            assert np.array_equal(_bits(res), first), variant  # the same arithmetic in every store path
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]


def test_survival_in_and_below_the_subnormal_range_is_inside_the_bound(gpu):
    """z of 708 to 745 gives a survival below 2^-1022, where fp64 is spaced 2^-1074 apart and the bound of coxsurvref
    carries that spacing in place of 2 u S*; beyond 745 the survival is 0.  Every row is still non-increasing."""
    X, cols, B, eta, delta = _curves_case()
    bt = np.arange(1.0, 65.0)
    bh = np.linspace(1.0, 2000.0, 64)
    ref = coxsurvref.curve_reference(eta, delta, bh, "survival")
    small = (ref["value"] < LD(2.0) ** -1022) & (ref["value"] > LD(2.0) ** -1074)
    assert int(small.sum()) >= 100 and (ref["value"] < LD(2.0) ** -1080).any() and (ref["value"] > 0.5).any()
    for variant in ("row-major", "column-major", "host"):
        _, view = _out(variant, N_CURVES, 64)
        got = gpu.cox_survival_device(_dev(X), cols, B, bt, bh, out=view).cpu().numpy()
        coxsurvref.check_curves(got, ref, "subnormal range, %s" % variant)
        assert (got[small] < 2.0 ** -1022).all() and (got[small] > 0).any() and (got == 0).any()
        assert (np.diff(got, axis=1) <= 0).all() and (got >= 0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_curves_read_every_layout_of_x_and_leave_it_unchanged(gpu, layout):
    n, T = 1025, 65
    for m in (0, 3, 70):
        X, cols, B, _, _ = _problem(n, m)
        t, vals = _view(X, layout)
        eta, delta = _eta(("edges", n, m, layout == "f32 row-major"), vals, cols, B)
        keep = t.clone()
        grid = _grid(T)
        got = gpu.cox_survival_device(t, cols, B, _BT, _BH, times=grid)
        ref = coxsurvref.curve_reference(eta, delta, gpu.baseline_at(_BT, _BH, grid), "survival")
        coxsurvref.check_curves(got.cpu().numpy(), ref, "%s m=%d" % (layout, m))
        assert torch.equal(t, keep)
        assert np.array_equal(_bits(gpu.cox_survival_device(t, cols, B, _BT, _BH, times=grid)), _bits(got))


def test_permuted_rows_give_permuted_bits_and_a_nan_stays_in_its_row(gpu):
    X, cols, B, eta, delta = _curves_case()
    n, T = N_CURVES, 65
    grid = _grid(T)
    hg = gpu.baseline_at(_BT, _BH, grid)
    clean = gpu.cox_survival_device(_dev(X), cols, B, _BT, _BH, times=grid).cpu().numpy()
    perm = np.random.default_rng(4).permutation(n)
    moved = gpu.cox_survival_device(_dev(X[perm]), cols, B, _BT, _BH, times=grid).cpu().numpy()
    assert np.array_equal(_bits(moved), _bits(clean[perm]))
    ref = coxsurvref.curve_reference(eta, delta, hg, "survival")
    for kind in ("survival", "cumhaz"):
        bad = X.copy()
        bad[321, cols[2]] = np.nan
        got = gpu.cox_survival_device(_dev(bad), cols, B, _BT, _BH, times=grid, kind=kind).cpu().numpy()
        assert np.isnan(got[321]).all() and not np.isnan(np.delete(got, 321, axis=0)).any()
        if kind == "survival":
            coxsurvref.check_curves(got, ref, "NaN in row 321", rows=np.arange(n) != 321)
            assert np.array_equal(_bits(np.delete(got, 321, axis=0)), _bits(np.delete(clean, 321, axis=0)))
    outside = X.copy()
    outside[:, np.setdiff1d(np.arange(P), cols)] = np.nan  # every column outside the support
    got = gpu.cox_survival_device(_dev(outside), cols, B, _BT, _BH, times=grid).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(clean))
    zero = np.append(B, 0.0)  # a coefficient that is exactly zero takes nothing from its column
    more = np.sort(np.append(cols, np.setdiff1d(np.arange(P), cols)[0])).astype(np.int32)
    Bz = np.zeros(more.size)
    Bz[np.searchsorted(more, cols)] = B
    got = gpu.cox_survival_device(_dev(outside), more, Bz, _BT, _BH, times=grid).cpu().numpy()
    assert not np.isnan(got).any() and zero[-1] == 0.0
    coxsurvref.check_curves(got, ref, "a NaN column with a zero coefficient")


def test_x_written_on_a_side_stream_just_before_the_calls_is_read_after_it(gpu):
    X, cols, B, time, status = _problem(4099, 3)
    grid = _grid(65)
    src = _dev(X)
    want_b = gpu.cox_baseline_device(src, cols, B, time, status)
    want_c = gpu.cox_survival_device(src, cols, B, _BT, _BH, times=grid)
    Xd = torch.zeros_like(src)
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(40):  # tens of milliseconds of work in front of the copy
            a = a @ a
            a = a / a.abs().max()
        Xd.copy_(src)
        handle = int(side.cuda_stream)
        got_c = gpu.cox_survival_device(Xd, cols, B, _BT, _BH, times=grid, stream=handle)
        got_b = gpu.cox_baseline_device(Xd, cols, B, time, status, stream=handle)
    assert np.array_equal(_bits(got_c), _bits(want_c))
    assert np.array_equal(_bits(got_b["cumhaz"]), _bits(want_b["cumhaz"]))
    torch.cuda.synchronize()


def test_c_abi_pointer_checks_ledger_and_bench(gpu):
    X, cols, B, time, status = _problem(64, 3)
    t = _dev(X)
    hg = np.array([0.0, 0.25, 0.5])
    lib = gpu.lib()
    before = gpu.process_counters()

    def curves(out_ptr, on_device, ors=3, ocs=1):
        a = gpu.CoxSurvivalInput()
        a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = t.data_ptr(), 0, P, 1, 64, P
        a.cols, a.m, a.B, a.hg, a.T, a.kind = gpu._ip(cols), 3, gpu._dp(B), gpu._dp(hg), 3, 0
        a.out_row_stride, a.out_col_stride, a.out_on_device = ors, ocs, on_device
        return lib.bessx_cox_survival_device(ctypes.byref(a), out_ptr)

    host = np.full((64, 3), -7.0)
    assert curves(host.ctypes.data, 1) == 1 and b"out" in lib.bessx_last_error()  # BESSX_ERR_ARG: a host pointer
    assert (host == -7.0).all()
    small = torch.zeros(32, dtype=torch.float64, device="cuda")
    assert curves(small.data_ptr(), 1, ors=1 << 24) == 1  # a device view that reaches past its allocation
    assert curves(host.ctypes.data, 0) == 0, gpu.last_error()
    eta, delta = _eta(("abi",), X, cols, B)
    coxsurvref.check_curves(host, coxsurvref.curve_reference(eta, delta, hg, "survival"), "C ABI, host out")
    assert (host[:, 0] == 1.0).all()
    strided = np.full((64, 7), -7.0)  # a host result at strides of its own
    assert curves(strided.ctypes.data, 0, ors=7, ocs=2) == 0, gpu.last_error()
    assert np.array_equal(_bits(strided[:, 0:6:2]), _bits(host)) and (strided[:, 1::2] == -7.0).all()
    a = gpu.CoxBaselineInput()
    a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = host.ctypes.data, 0, P, 1, 64, P  # x: a host pointer
    a.cols, a.m, a.B = gpu._ip(cols), 3, gpu._dp(B)
    a.time, a.status = gpu._dp(time), gpu._dp(status)
    J, times, cumhaz = ctypes.c_int(-7), np.zeros(64), np.zeros(64)
    assert lib.bessx_cox_baseline_device(ctypes.byref(a), ctypes.byref(J), gpu._dp(times), gpu._dp(cumhaz)) == 1
    a.x = t.data_ptr()
    assert lib.bessx_cox_baseline_device(ctypes.byref(a), ctypes.byref(J), gpu._dp(times), gpu._dp(cumhaz)) == 0
    ref = coxsurvref.baseline_reference(eta, delta, time, status, None)
    coxsurvref.check_baseline(times[:J.value], cumhaz[:J.value], ref, "C ABI baseline")
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
    assert after["allocation_requests"] > before["allocation_requests"]
    for col_major in (False, True):
        ms = gpu.op_cox_surv_bench(t, cols, T=5, out_col_major=col_major, repeats=2)
        assert len(ms) == 3 and all(v > 0 for v in ms)
    assert gpu.process_counters()["live_device_bytes"] == before["live_device_bytes"]


# ----------------------------------------------------------------------------------------------------------------
# the estimator
# ----------------------------------------------------------------------------------------------------------------
def test_the_estimator_against_the_capi_route_and_the_numpy_route(gpu):
    X, obs, status, _, _ = synth.make_cox(300, 20, 3, seed=76)
    y = np.column_stack([obs, status])
    Xd = _dev(X)
    est = linear.PdasCox(sequence=[1, 2, 3, 4])
    est.fit(Xd, y)
    assert not hasattr(est, "baseline_times_")  # (fit() does not compute the baseline)
    with pytest.raises(ValueError, match="fit_baseline"):
        est.predict_survival(Xd)
    w = np.random.default_rng(7).integers(1, 17, 300) / 8.0
    cols = np.nonzero(est.beta)[0]
    assert cols.size > 0
    eta, delta = evalref.eta_reference(X, cols, est.beta[cols].reshape(-1, 1), [0.0])
    eta, delta = eta[:, 0], delta[:, 0]
    host = linear.PdasCox()
    host.p, host.beta, host.coef0 = est.p, est.beta, est.coef0
    for wt in (None, w):
        assert est.fit_baseline(Xd, _dev(y), weight=None if wt is None else _dev(wt)) is est
        base = gpu.cox_baseline_device(Xd, cols, est.beta[cols], obs, status, weight=wt)
        assert np.array_equal(_bits(est.baseline_times_), _bits(base["times"]))
        assert np.array_equal(_bits(est.baseline_cumhaz_), _bits(base["cumhaz"]))
        ref = coxsurvref.baseline_reference(eta, delta, obs, status, wt)
        coxsurvref.check_baseline(est.baseline_times_, est.baseline_cumhaz_, ref, "estimator, device")
        host.fit_baseline(X, y, weight=wt)
        coxsurvref.check_baseline(host.baseline_times_, host.baseline_cumhaz_, ref, "estimator, numpy")
        for kind in ("survival", "cumhaz"):
            got = est.predict_survival(Xd, kind=kind)
            assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (300, base["times"].size)
            direct = gpu.cox_survival_device(Xd, cols, est.beta[cols], base["times"], base["cumhaz"], kind=kind)
            assert np.array_equal(_bits(got), _bits(direct))
            # each route is inside its bound of the exact curves (its H0 inside the baseline's bound): they agree
            # within the sum of the two
            cref = coxsurvref.curve_reference(eta, delta, ref["cumhaz"], kind, hg_bound=ref["bound"])
            coxsurvref.check_curves(got.cpu().numpy(), cref, "estimator, device")
            other = host.predict_survival(X, kind=kind)
            coxsurvref.check_curves(other, cref, "estimator, numpy")
            assert (np.abs(got.cpu().numpy().astype(LD) - other.astype(LD)) <= 2 * cref["bound"]).all()
        surv = est.predict_survival(Xd).cpu().numpy()
        assert (np.diff(surv, axis=1) <= 0).all() and (surv >= 0).all() and (surv <= 1).all()
    some = est.predict_survival(Xd, times=[obs.max() + 1.0, obs.min() - 1.0])
    assert tuple(some.shape) == (300, 2) and bool((some[:, 1] == 1.0).all()) and bool((some[:, 0] < 1.0).all())
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 20"):
        est.predict_survival(Xd[:, :19])
