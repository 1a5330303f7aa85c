"""Standard errors and confidence bands of Cox survival curves on an X already in GPU memory (bessx_cox_hazard_var_device,
bessx_cox_band_device, bess_amd/csrc/bessx_k_coxband.hip) against NumPy in np.longdouble on the host copy of the same
values.  The bounds are derived in tests/coxbandref.py; every check prints error against bound, and every case that is not
marked adversarial also asserts that the bound itself is at most 1e-9.  The shapes are the smallest that reach every path:
the 1024-position scan blocks of step 1; for step 2 the 16-row (element loads), 32-row (16-byte loads, fp64) and 64-row
(16-byte loads, fp32) workgroups, one, two and five 16-column output tiles, more than one run of tiles (m = 1023), and
the time chunks of k_cbd_band: 16 grid times per workgroup for element loads, 8 for 16-byte loads of fp64, 4 for 16-byte
loads of fp32 -- T runs over 1, 2 and one below / at / above each of 4, 8 and 16."""
import ctypes

import numpy as np
import pytest

import coxbandref
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
    """test_cox_surv_gpu.py's: X (n x P, N(0, 1)), m ascending support columns with coefficients N(0, 1 / m), continuous
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


LAYOUTS = ["f64 row-major", "f64 column-major", "f32 row-major", "strided"]  # (test_cox_surv_gpu.py's four)
LAYOUTS2 = LAYOUTS + ["f32 column-major"]  # (step 2: the 16-byte loads of fp32 have a time chunk of their own)
CHUNK = {"f64 row-major": 16, "f64 column-major": 8, "f32 row-major": 16, "strided": 16, "f32 column-major": 4}


def _view(vals, layout):
    """(the n x P device view of the values in the given layout, the widened values it holds); every padding is NaN"""
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
    if layout == "f32 column-major":
        v32 = vals.astype(np.float32)
        F = np.full((p, (n + 7) // 8 * 8), np.nan, dtype=np.float32)
        F[:, :n] = v32.T
        return _dev(F)[:, :n].T, v32.astype(np.float64)
    S = np.full((2 * n, 3 * p), np.nan)  # both strides > 1
    S[::2, 1::3] = vals
    return _dev(S)[::2, 1::3], vals


def _time_grid(time, status):
    """before the first / between / at / after the last event time, unsorted, with repeats"""
    ev = np.sort(time[status != 0])
    if ev.size == 0:
        return np.array([time.min() - 1.0, time.max() + 1.0])
    mid = 0.5 * (ev[ev.size // 2] + ev[ev.size // 2 - 1]) if ev.size > 1 else ev[0] + 0.25
    g = np.array([ev[-1] + 1.0, ev[0] - 0.5, mid, ev[ev.size // 3], ev[-1], ev[0], mid, time.max(), np.median(time)])
    return g[np.random.default_rng(ev.size).permutation(g.size)]


# ----------------------------------------------------------------------------------------------------------------
# step 1: cumhaz, var0, drift
# ----------------------------------------------------------------------------------------------------------------
def _hv_ref(key, vals, cols, B, time, status, w, ties, grid):
    if key not in _REFS:
        _REFS[key] = coxbandref.hazard_var_reference(vals, cols, B, time, status, w, ties, grid)
    return _REFS[key]


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049])
def test_hazard_var_at_the_block_edges_for_every_layout_and_support(gpu, n):
    for m in (0, 1, 3, 70):
        X, cols, B, time, status = _problem(n, m)
        if n <= 2:
            status = np.ones(n)
        grid = _time_grid(time, status)
        for layout in LAYOUTS:
            t, vals = _view(X, layout)
            f32 = layout == "f32 row-major"
            cases = (("breslow", "none"),)
            if layout == "f64 row-major":
                cases = (("breslow", "none"), ("order", "random"), ("breslow", "zeros")) if m == 3 else \
                        (("breslow", "none"), ("order", "none"))
            for ties, wk in cases:
                w = _weights(n, wk)
                ref = _hv_ref(("edges", n, m, f32, ties, wk), vals, cols, B, time, status, w, ties, grid)
                got = gpu.cox_baseline_variance_device(t, cols, B, time, status, grid, weight=w, ties=ties)
                assert set(got) == {"times", "cumhaz", "var0", "drift", "n_events"}
                assert got["drift"].shape == (grid.size, m) and np.array_equal(got["times"], grid)
                coxbandref.check_hazard_var(got, ref, "n=%d m=%d %s %s w=%s" % (n, m, layout, ties, wk))
                assert got["n_events"] == float(np.sum(status if w is None else w * status))
                if ties == "breslow":  # the launchers are shared: the baseline's bits
                    base = gpu.cox_baseline_device(t, cols, B, time, status, weight=w)
                    want = gpu.baseline_at(base["times"], base["cumhaz"], grid)
                    assert np.array_equal(_bits(got["cumhaz"]), _bits(want)), (n, m, layout)
        again = gpu.cox_baseline_variance_device(t, cols, B, time, status, grid, weight=w, ties=ties)
        for k in ("cumhaz", "var0", "drift"):
            assert np.array_equal(_bits(again[k]), _bits(got[k])), k


def test_hazard_var_with_a_tie_group_across_a_block_boundary_and_without_events(gpu):
    n, m = 2049, 3
    X, cols, B, _, status = _problem(n, m)
    rows = np.random.default_rng(3).permutation(n)  # rows[k]: the row at position k
    tpos = np.arange(n, dtype=np.float64)
    tpos[1020:1031] = 1020.0  # one tie group over positions 1020..1030
    time = np.empty(n)
    time[rows] = tpos
    status[rows[1020:1031]] = 1.0
    grid = np.array([1020.0, 1019.5, 1030.0, 1031.0, -1.0, 1020.0, 5000.0, 1023.0])
    t = _dev(X)
    for ties in ("breslow", "order"):
        for wk in ("none", "zeros"):
            w = _weights(n, wk)
            ref = coxbandref.hazard_var_reference(X, cols, B, time, status, w, ties, grid)
            got = gpu.cox_baseline_variance_device(t, cols, B, time, status, grid, weight=w, ties=ties)
            coxbandref.check_hazard_var(got, ref, "tie group over a block boundary, %s w=%s" % (ties, wk))
            assert got["cumhaz"][4] == 0.0 and got["var0"][4] == 0.0 and (got["drift"][4] == 0.0).all()
            for k in ("cumhaz", "var0", "drift"):  # 1020, 1023 and 1030 are the same tie group's end
                assert np.array_equal(_bits(got[k][0]), _bits(got[k][2])) and np.array_equal(_bits(got[k][0]), _bits(got[k][7]))
    none = gpu.cox_baseline_variance_device(t, cols, B, time, np.zeros(n), grid)
    assert none["n_events"] == 0.0 and not none["cumhaz"].any() and not none["var0"].any() and not none["drift"].any()


# ----------------------------------------------------------------------------------------------------------------
# step 2: the bands, from synthetic cumhaz / var0 / drift and a synthetic lower-triangular R
# ----------------------------------------------------------------------------------------------------------------
def _synthetic(m, T, seed=17, shift=0.0):
    """cumhaz (T,) from 0 up, var0, drift (T, m) about cumhaz * (shift + noise), R (m, m) lower triangular with a
    NaN strict upper triangle (never read)"""
    rng = np.random.default_rng(seed + 3 * m + T)
    H = np.concatenate([[0.0], np.cumsum(rng.uniform(0.02, 0.2, T))])[:T] if T > 1 else np.array([0.37])
    H = H[rng.permutation(T)]
    V0 = H * H / 40.0 + H / 300.0
    D = H[:, None] * (shift + 0.3 * rng.standard_normal((T, m)))
    R = np.tril(0.3 * rng.standard_normal((m, m)) / np.sqrt(max(m, 1))) + 0.4 * np.eye(m)
    R[np.triu_indices(m, 1)] = np.nan
    return H, V0, D, R


def _beta(m, seed=23):
    return np.random.default_rng(seed + m).standard_normal(m) / np.sqrt(max(m, 1))


KC = [("survival", "log-log"), ("survival", "log"), ("survival", "plain"), ("cumhaz", "log"), ("cumhaz", "plain")]


def _check(gpu, t, vals, cols, B, H, V0, D, R, kind, conf, what_, msg, level=0.95, ordinary=True, rows=None):
    got = gpu.cox_survival_band_device(t, cols, B, H, V0, D, R, kind=kind, conf_type=conf, level=level, what=what_)
    ref = coxbandref.band_reference(vals, cols, B, H, V0, D, R, kind, conf, gpu.normal_quantile(level),
                                    coxbandref.device_depths(len(cols)))
    host = {k: v.cpu().numpy() for k, v in got.items()}
    coxbandref.check_bands(host, ref, list(got), msg, ordinary=ordinary, rows=rows)
    z = H == 0.0
    if z.any() and rows is None and all(k in host for k in coxbandref.WHAT):
        assert (host["se"][:, z] == 0.0).all()
        assert np.array_equal(_bits(host["lower"][:, z]), _bits(host["estimate"][:, z]))
        assert np.array_equal(_bits(host["upper"][:, z]), _bits(host["estimate"][:, z]))
    return got, host


@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 65])
def test_bands_at_the_row_tile_edges_for_every_support_and_layout(gpu, n):
    T = 9
    for im, m in enumerate((0, 1, 3, 15, 16, 17, 70)):
        X, cols, _, _, _ = _problem(n, m)
        B = _beta(m)
        H, V0, D, R = _synthetic(m, T)
        for il, layout in enumerate(LAYOUTS2):
            t, vals = _view(X, layout)
            kind, conf = KC[(im + il) % len(KC)]
            _, host = _check(gpu, t, vals, cols, B, H, V0, D, R, kind, conf, coxbandref.WHAT,
                             "n=%d m=%d %s %s %s" % (n, m, layout, kind, conf))
            assert (host["lower"] <= host["estimate"]).all() and (host["estimate"] <= host["upper"]).all()
            assert (host["lower"] >= 0.0).all() and (kind == "cumhaz" or (host["upper"] <= 1.0).all())


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33])
def test_bands_at_the_time_chunk_edges_of_every_access_shape(gpu, T):
    n, m = 33, 17
    X, cols, _, _, _ = _problem(n, m)
    B = _beta(m)
    H, V0, D, R = _synthetic(m, T)
    for il, layout in enumerate(LAYOUTS2):
        t, vals = _view(X, layout)
        dx = gpu._DeviceArray(t, "x", 2)
        assert gpu.cox_band_workspace(n, m, T, dtype=np.float32 if "f32" in layout else np.float64,
                                      row_stride=dx.strides[0], col_stride=dx.strides[1])[1] == CHUNK[layout]
        for kind, conf in KC:
            _check(gpu, t, vals, cols, B, H, V0, D, R, kind, conf, coxbandref.WHAT, "T=%d %s %s %s" % (T, layout, kind, conf))


def test_bands_at_the_largest_support(gpu):
    n, m, T = 33, 1023, 5
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, m + 1))
    cols = np.delete(np.arange(m + 1), 500).astype(np.int32)
    B = _beta(m)
    H, V0, D, R = _synthetic(m, T)
    for layout in ("f64 column-major", "f64 row-major", "f32 column-major"):
        t, vals = _view(X, layout)
        _check(gpu, t, vals, cols, B, H, V0, D, R, "survival", "log-log", coxbandref.WHAT, "m=1023 %s" % layout)


def test_every_subset_size_of_what_and_every_kind_of_out(gpu):
    n, m, T = 33, 17, 9
    X, cols, _, _, _ = _problem(n, m)
    B = _beta(m)
    H, V0, D, R = _synthetic(m, T)
    t = _dev(X)
    full = gpu.cox_survival_band_device(t, cols, B, H, V0, D, R, what=coxbandref.WHAT)
    assert list(full) == list(coxbandref.WHAT)
    base = full["estimate"]._base if full["estimate"]._base is not None else full["estimate"]
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and tuple(v.shape) == (n, T) for v in full.values())
    assert tuple(base.shape) == (4, n, T)  # (views of one tensor)
    before = gpu.process_counters()
    for names in (("se",), ("upper", "estimate"), ("lower", "se", "upper"), coxbandref.WHAT):
        got = gpu.cox_survival_band_device(t, cols, B, H, V0, D, R, what=names)
        assert list(got) == [k for k in coxbandref.WHAT if k in names]
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(full[k])), (names, k)
        K = len(names)
        # out given: slabs, rows and columns all at non-unit strides; the bytes outside the view stay untouched
        buf = torch.full((K, 2, n + 1, 2 * T + 1), -7.0, dtype=torch.float64, device="cuda")
        view = buf[:, 1, :n, 1:2 * T:2]
        res = gpu.cox_survival_band_device(t, cols, B, H, V0, D, R, what=names, out=view)
        for s, k in enumerate(got):
            assert np.array_equal(_bits(view[s]), _bits(full[k])) and np.array_equal(_bits(res[k]), _bits(full[k]))
        view.fill_(-7.0)
        assert bool((buf == -7.0).all())
        colmajor = torch.full((K, T, n), -7.0, dtype=torch.float64, device="cuda")
        gpu.cox_survival_band_device(t, cols, B, H, V0, D, R, what=names, out=colmajor.permute(0, 2, 1))
        for s, k in enumerate(got):
            assert np.array_equal(_bits(colmajor[s].T), _bits(full[k]))

    class Plain:  # a device array that is not a torch tensor: the result is a host array
        __cuda_array_interface__ = t.__cuda_array_interface__

    host = gpu.cox_survival_band_device(Plain(), cols, B, H, V0, D, R, what=("lower", "upper"))
    assert all(isinstance(v, np.ndarray) and v.shape == (n, T) for v in host.values())
    assert np.array_equal(_bits(host["lower"]), _bits(full["lower"])) and np.array_equal(_bits(host["upper"]), _bits(full["upper"]))
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]


def test_columns_that_are_not_centred_stay_inside_the_derived_bound(gpu):
    """Columns shifted by +50: p_tau is about cumhaz * R xbar, so p - cumhaz t cancels and the expansion |p|^2 - 2 H p.t +
    H^2 |t|^2 would lose the digits twice.  Adversarial for the 1e-9 condition, still inside the derived bound."""
    n, m, T = 65, 17, 9
    X, cols, _, _, _ = _problem(n, m)
    X = X + 50.0
    B = _beta(m) / 50.0
    H, V0, D, R = _synthetic(m, T, shift=50.0)
    for layout in LAYOUTS2:
        t, vals = _view(X, layout)
        for kind, conf in KC:
            _check(gpu, t, vals, cols, B, H, V0, D, R, kind, conf, coxbandref.WHAT, "shifted by 50, %s %s %s" % (layout, kind, conf),
                   ordinary=False)


def test_a_rows_bits_do_not_depend_on_layout_position_or_n(gpu):
    """V(i, .) is formed from row i's values and the T-sized inputs alone.  e_i comes from section 2f's predictor pass, kept
    as it is so that estimate has cox_survival_device's bits: for a row-contiguous X that pass adds the support's products
    in another order than for the other layouts.  So: with beta = 0 (e = 1 exactly, t = R z still in play) every fp64
    layout gives the same bits; with beta != 0 the layouts that share the predictor's route do; and under one layout a
    row's bits do not depend on where the row lies or on n."""
    n, m, T = 65, 17, 9
    X, cols, _, _, _ = _problem(n, m)
    H, V0, D, R = _synthetic(m, T)
    f64 = ("f64 row-major", "f64 column-major", "strided")
    zero = {L: gpu.cox_survival_band_device(_view(X, L)[0], cols, np.zeros(m), H, V0, D, R, what=coxbandref.WHAT) for L in f64}
    for L in f64[1:]:
        for k in coxbandref.WHAT:
            assert np.array_equal(_bits(zero[L][k]), _bits(zero[f64[0]][k])), (L, k)
    assert float(zero[f64[0]]["se"].max()) > 0.0
    B = _beta(m)
    got = {L: gpu.cox_survival_band_device(_view(X, L)[0], cols, B, H, V0, D, R, what=coxbandref.WHAT) for L in f64}
    for k in coxbandref.WHAT:
        assert np.array_equal(_bits(got["strided"][k]), _bits(got["f64 column-major"][k])), k
    perm = np.random.default_rng(4).permutation(n)
    big = np.vstack([np.random.default_rng(6).standard_normal((37, P)), X[perm], np.random.default_rng(7).standard_normal((100, P))])
    for L in f64:
        moved = gpu.cox_survival_band_device(_view(big, L)[0], cols, B, H, V0, D, R, what=coxbandref.WHAT)
        for k in coxbandref.WHAT:
            assert np.array_equal(_bits(moved[k][37:37 + n]), _bits(got[L][k][perm])), (L, k)


def test_a_nan_stays_in_its_row_and_nothing_outside_the_support_is_read(gpu):
    n, m, T = 65, 17, 9
    X, cols, _, _, _ = _problem(n, m)
    B = _beta(m)
    H, V0, D, R = _synthetic(m, T)
    for layout in LAYOUTS2:  # (the paddings of _view are NaN: a read of one would show)
        t, vals = _view(X, layout)
        clean = gpu.cox_survival_band_device(t, cols, B, H, V0, D, R, what=coxbandref.WHAT)
        bad = X.copy()
        bad[40, cols[5]] = np.nan
        bad[:, np.setdiff1d(np.arange(P), cols)] = np.nan  # every column outside the support
        got = gpu.cox_survival_band_device(_view(bad, layout)[0], cols, B, H, V0, D, R, what=coxbandref.WHAT)
        for k in coxbandref.WHAT:
            g, c = got[k].cpu().numpy(), clean[k].cpu().numpy()
            assert np.isnan(g[40]).all(), (layout, k)
            assert np.array_equal(_bits(np.delete(g, 40, axis=0)), _bits(np.delete(c, 40, axis=0))), (layout, k)


def test_estimate_has_the_bits_of_cox_survival_device(gpu):
    n, T = 65, 17
    for m in (0, 3, 70):
        X, cols, _, _, _ = _problem(n, m)
        B = _beta(m)
        H, V0, D, R = _synthetic(m, T)
        bt = np.arange(1.0, T + 1.0)
        order = np.argsort(H, kind="stable")  # (a baseline is ascending: the step-function lookup returns H itself)
        for layout in LAYOUTS2:
            t, _ = _view(X, layout)
            for kind in ("survival", "cumhaz"):
                got = gpu.cox_survival_band_device(t, cols, B, H, V0, D, R, kind=kind, conf_type="plain", what=("estimate",))
                inv = np.empty(T)
                inv[order] = bt
                want = gpu.cox_survival_device(t, cols, B, bt, H[order], times=inv, kind=kind)
                assert np.array_equal(_bits(got["estimate"]), _bits(want)), (m, layout, kind)


# ----------------------------------------------------------------------------------------------------------------
# the estimator, end to end
# ----------------------------------------------------------------------------------------------------------------
def test_the_estimator_against_the_reference_and_the_numpy_route(gpu):
    n, m, T = 2049, 8, 65
    X, cols, _, time, status = _problem(n, m)
    beta = np.zeros(P)
    beta[cols] = _beta(m)
    y = np.column_stack([time, status])
    grid = np.concatenate([_time_grid(time, status), np.random.default_rng(8).uniform(0.0, 3.0, T - 9)])
    est, host = linear.PdasCox(), linear.PdasCox()
    for e in (est, host):
        e.p, e.beta, e.coef0 = P, beta, 0.0
    Xd = _dev(X)
    with pytest.raises(ValueError, match="fit_survival_bands"):
        est.predict_survival_bands(Xd)
    assert est.fit_survival_bands(Xd, _dev(y), grid) is est
    host.fit_survival_bands(X, y, grid)
    ref = coxbandref.hazard_var_reference(X, cols, beta[cols], time, status, None, "breslow", grid)
    for e, what_ in ((est, "device"), (host, "numpy")):
        coxbandref.check_hazard_var({"cumhaz": e.band_cumhaz_, "var0": e.band_var0_, "drift": e.band_drift_}, ref,
                                    "estimator, " + what_)
        assert e.band_factor_.shape == (m, m) and np.array_equal(e.band_times_, grid)
    Xn = np.random.default_rng(10).standard_normal((257, P))
    zc = gpu.normal_quantile(0.95)
    for kind, conf in KC:
        got = est.predict_survival_bands(_dev(Xn), kind=kind, conf_type=conf, what=coxbandref.WHAT)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and tuple(v.shape) == (257, T) for v in got.values())
        other = host.predict_survival_bands(Xn, kind=kind, conf_type=conf, what=coxbandref.WHAT)
        for e, res, depths, what_ in ((est, {k: v.cpu().numpy() for k, v in got.items()}, coxbandref.device_depths(m), "device"),
                                      (host, other, coxbandref.host_depths(m), "numpy")):
            # each route against the exact values, with the bounds of what it holds in their place and its own factor
            r = coxbandref.band_reference(Xn, cols, beta[cols], ref["cumhaz"], ref["var0"], ref["drift"], e.band_factor_,
                                          kind, conf, zc, depths,
                                          in_bounds=(ref["cumhaz_bound"], ref["var0_bound"], ref["drift_bound"]))
            coxbandref.check_bands(res, r, coxbandref.WHAT, "estimator, %s %s %s" % (what_, kind, conf))


# ----------------------------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------------------------
def test_c_abi_limits_pointer_checks_and_ledger(gpu):
    n, m, T = 64, 3, 3
    X, cols, _, time, status = _problem(n, m)
    B = _beta(m)
    H, V0, D, R = _synthetic(m, T)
    R = np.tril(np.nan_to_num(R))
    t = _dev(X)
    lib = gpu.lib()
    before = gpu.process_counters()

    def band(out_ptr, on_device, x_ptr=None, mm=None, **kw):
        a = gpu.CoxBandInput()
        a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = x_ptr or t.data_ptr(), 0, P, 1, n, P
        a.cols, a.m, a.beta = gpu._ip(cols), m if mm is None else mm, gpu._dp(B)
        a.cumhaz, a.var0, a.drift, a.drift_ld, a.T = gpu._dp(H), gpu._dp(V0), gpu._dp(D), m, T
        a.factor, a.factor_ld, a.kind, a.conf_type, a.z_c, a.what = gpu._dp(R), m, 0, 2, 1.96, 15
        a.out_slab_stride, a.out_row_stride, a.out_col_stride, a.out_on_device = n * T, T, 1, on_device
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.bessx_cox_band_device(ctypes.byref(a), out_ptr)

    host = np.full((4, n, T), -7.0)
    assert band(host.ctypes.data, 1) == 1 and b"out" in lib.bessx_last_error()  # BESSX_ERR_ARG: a host pointer as device out
    assert band(host.ctypes.data, 0, x_ptr=host.ctypes.data) == 1 and b"x" in lib.bessx_last_error()  # x: a host pointer
    assert (host == -7.0).all()
    small = torch.zeros(32, dtype=torch.float64, device="cuda")
    assert band(small.data_ptr(), 1, out_row_stride=1 << 24) == 1  # a device view that reaches past its allocation
    assert band(small.data_ptr(), 1, out_slab_stride=1 << 30) == 1  # ... by its second slab only
    assert bool((small == 0.0).all())
    for kw in ({"kind": 2}, {"conf_type": 3}, {"kind": 1, "conf_type": 2}, {"what": 0}, {"what": 16}, {"z_c": -1.0},
               {"z_c": float("nan")}, {"T": 0}, {"out_row_stride": -1}, {"out_col_stride": 0}, {"drift_ld": m - 1},
               {"factor_ld": m - 1}):
        assert band(host.ctypes.data, 0, **kw) == 1, kw
    assert band(host.ctypes.data, 0, T=65536) == 3  # BESSX_ERR_UNSUPPORTED
    wide, zeros = np.arange(1024, dtype=np.int32), np.zeros(1024)  # m + 1 > 1024 (found before anything is read)
    big = dict(cols=gpu._ip(wide), beta=gpu._dp(zeros), p=2000)
    assert band(host.ctypes.data, 0, mm=1024, **big) == 3 and b"1024" in lib.bessx_last_error()
    assert (host == -7.0).all()
    assert band(host.ctypes.data, 0) == 0, gpu.last_error()
    ref = coxbandref.band_reference(X, cols, B, H, V0, D, R, "survival", "log-log", 1.96, coxbandref.device_depths(m))
    coxbandref.check_bands(dict(zip(coxbandref.WHAT, host)), ref, coxbandref.WHAT, "C ABI, host out")

    def hazvar(x_ptr, mm=None, **kw):
        a = gpu.CoxHazardVarInput()
        a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = x_ptr, 0, P, 1, n, P
        a.cols, a.m, a.beta = gpu._ip(cols), m if mm is None else mm, gpu._dp(B)
        a.time, a.status, a.ties = gpu._dp(time), gpu._dp(status), 1
        grid = np.array([0.5, 1.0, 0.25])
        a.times, a.T = gpu._dp(grid), 3
        for k, v in kw.items():
            setattr(a, k, v)
        c, v, d, ne = np.zeros(3), np.zeros(3), np.zeros((3, m)), ctypes.c_double(0)
        return lib.bessx_cox_hazard_var_device(ctypes.byref(a), gpu._dp(c), gpu._dp(v), gpu._dp(d), m, ctypes.byref(ne)), c

    assert hazvar(host.ctypes.data)[0] == 1  # x: a host pointer
    assert hazvar(t.data_ptr(), mm=1024, **big)[0] == 3
    assert hazvar(t.data_ptr(), ties=2)[0] == 1 and hazvar(t.data_ptr(), T=0)[0] == 1
    nan = np.array([0.5, np.nan, 1.0])
    assert hazvar(t.data_ptr(), times=gpu._dp(nan))[0] == 1 and b"NaN" in lib.bessx_last_error()
    rc, c = hazvar(t.data_ptr())
    assert rc == 0 and c[1] >= c[0] >= c[2] > 0.0
    nd = ctypes.c_longlong(0)
    assert lib.bessx_cox_hazard_var_workspace(n, m, int(status.sum()), 3, ctypes.byref(nd)) == 0 and nd.value > n * m
    assert lib.bessx_cox_hazard_var_workspace(n, 1024, 1, 3, ctypes.byref(nd)) == 3
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
    assert after["allocation_requests"] > before["allocation_requests"]
