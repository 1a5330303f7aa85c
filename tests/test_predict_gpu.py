"""Prediction on an X already in GPU memory (bessx_predict_device, bess_amd/csrc/bessx_k_predict.hip) against NumPy in
np.longdouble on the host copy of the same values.

The bound on the linear predictor is derived, not measured: for row i and response r

    |eta_hat - eta*| <= gamma * (|c_r| + sum_j |x_ij| |B_jr|),   gamma = (m + 2) u / (1 - (m + 2) u),   u = 2^-53,

the standard bound for an m-term dot product plus one addition in any summation order, with or without fused
multiply-add (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Call the right-hand side Delta.
  pr   within Delta / 4 + 8 u absolute: |d pr / d eta| <= 1/4; 8 u covers exp (at most 1 ulp in double), one addition and
       one division on values <= 1
  lam  within Delta + 8 u relative
  labels equal (eta* > 0) on every row, after asserting that no row has |eta*| <= Delta
Where two routes are compared with each other (device against host NumPy) each is within its bound of the exact value,
so they agree within twice that bound."""
import ctypes

import numpy as np
import pytest

from bess_amd import linear, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
U = LD(2.0) ** -53
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
P = 600
NS, MS, RS = (1, 127, 4097), (0, 1, 7, 200, P), (1, 5, 256)


def _cases():
    """Every n with every m at R = 5; every R at n = 1 and 127 with every m, and at n = 4097 with m = 7 and 200 (the
    longdouble reference of the full cross product would take minutes); R = 3 on top (the four-response tile)."""
    out = []
    for n in NS:
        for m in MS:
            for R in RS:
                if R == 5 or n <= 127 or m in (7, 200):
                    out.append((n, m, R))
    return out + [(127, 7, 3), (127, 200, 3)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _design(rng, shape, npdt):
    """Mixed signs, column scales 1e-6 .. 1e6 (along the LAST axis of `shape` when transposed later: scales per entry)."""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(npdt)


def _view(layout, n, p, npdt, rng):
    """(base host array, function base tensor -> the n x p view under test, the view's values on the host)"""
    if layout == "C":  # row-major
        b = _design(rng, (n, p), npdt)
        return b, (lambda t: t), b
    if layout == "F":  # column-major with a padded leading dimension: aligned columns (the 16-byte loads)
        ldn = (n + 3) // 4 * 4
        b = _design(rng, (p, ldn), npdt)
        return b, (lambda t: t[:, :n].T), b[:, :n].T
    if layout == "T":  # a transposed view that starts on an odd element: column-contiguous, element loads
        b = _design(rng, (p, n + 3), npdt)
        return b, (lambda t: t[:, 1:1 + n].T), b[:, 1:1 + n].T
    if layout == "two_strides":
        b = _design(rng, (2 * n, 3 * p), npdt)
        return b, (lambda t: t[::2, ::3]), b[::2, ::3]
    if layout == "odd_offset":  # row-contiguous, first element at an odd offset
        b = _design(rng, (n, p + 5), npdt)
        return b, (lambda t: t[:, 3:3 + p]), b[:, 3:3 + p]
    raise AssertionError(layout)


def _model(rng, p, m, R, scales=True):
    cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
    B = rng.standard_normal((m, R))
    c = rng.standard_normal(R)
    if scales:
        B *= 10.0 ** rng.uniform(-6, 6, (m, R))
        c *= 10.0 ** rng.uniform(-6, 6, R)
    return cols, B, c


def _reference(vals, cols, B, c):
    """(eta*, Delta) in longdouble for the widened values of the view, both (n, R)."""
    Xs = np.asarray(vals)[:, cols].astype(LD)
    cl = np.asarray(c, dtype=LD).reshape(-1)
    Bl = np.asarray(B, dtype=LD).reshape(len(cols), cl.size)
    eta = Xs @ Bl + cl[None, :]
    k = LD(len(cols) + 2) * U
    delta = k / (LD(1) - k) * (np.abs(Xs) @ np.abs(Bl) + np.abs(cl)[None, :])
    return eta, delta


def _host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_host(a)).view(np.int64)


def _check_eta(got, eta, delta, what):
    err = np.abs(_host(got).astype(LD).reshape(eta.shape) - eta)
    worst = float(np.max(err - delta))
    print("%s: max |err| %.3e, max Delta %.3e, max (err - Delta) %.3e" % (what, float(err.max()), float(delta.max()),
                                                                            worst))
    assert np.isfinite(_host(got)).all(), what
    assert (err <= delta).all(), (what, worst)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_linear_predictor_is_within_the_dot_product_bound(gpu, dt, layout):
    rng = np.random.default_rng(2024)
    for n in NS:
        base, view, vals = _view(layout, n, P, DT[dt], rng)
        tb = _dev(base)
        t = view(tb)
        assert tuple(t.shape) == (n, P)
        for (n_, m, R) in _cases():
            if n_ != n:
                continue
            cols, B, c = _model(rng, P, m, R)
            eta, delta = _reference(vals, cols, B, c)
            got = gpu.predict_device(t, cols, B, c)
            assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (n, R)
            assert got.dtype == torch.float64
            _check_eta(got, eta, delta, "%s %s n=%d m=%d R=%d" % (dt, layout, n, m, R))
            if m == 0:
                assert np.array_equal(_host(got), np.broadcast_to(c, (n, R)))  # every row gets c
            again = gpu.predict_device(t, cols, B, c)
            assert np.array_equal(_bits(got), _bits(again)), "the same call twice must give the same bits"
        ibits = np.int64 if dt == "f64" else np.int32
        assert np.array_equal(tb.cpu().numpy().view(ibits), base.view(ibits))  # X is never written


def test_one_dimensional_coefficients_give_a_vector_and_numpy_for_other_device_objects(gpu):
    class Plain:  # a device object that is no torch tensor
        def __init__(self, t):
            self._t, self.__cuda_array_interface__ = t, t.__cuda_array_interface__

    rng = np.random.default_rng(5)
    vals = _design(rng, (300, 40), np.float64)
    t = _dev(vals)
    cols, B, c = _model(rng, 40, 9, 1)
    eta, delta = _reference(vals, cols, B, c)
    got = gpu.predict_device(t, cols, B[:, 0], c)
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (300,)
    _check_eta(got, eta, delta, "1-D coefficients")
    host = gpu.predict_device(Plain(t), cols, B, c)  # staged through the library's device buffer, copied back
    assert isinstance(host, np.ndarray) and host.shape == (300, 1)
    assert np.array_equal(_bits(host), _bits(got).reshape(300, 1))
    pr, lab = gpu.predict_device(Plain(t), cols, B * 1e-3, c * 0, link="logistic")
    pr_d, lab_d = gpu.predict_device(t, cols, B * 1e-3, c * 0, link="logistic")
    assert np.array_equal(_bits(pr), _bits(pr_d)) and np.array_equal(_bits(lab), _bits(lab_d))


def test_nan_in_a_support_column_reaches_its_row_only(gpu):
    rng = np.random.default_rng(6)
    vals = rng.standard_normal((200, 30))
    vals[17, 4] = np.nan   # a support column
    vals[23, 5] = np.nan   # not in the support: never read
    cols = np.array([1, 4, 9], dtype=np.int32)
    B, c = rng.standard_normal((3, 2)), rng.standard_normal(2)
    for t in (_dev(vals), _dev(vals.T).T):
        got = _host(gpu.predict_device(t, cols, B, c))
        assert np.isnan(got[17]).all() and np.isfinite(np.delete(got, 17, axis=0)).all()
        pr, lab = (_host(a) for a in gpu.predict_device(t, cols, B, c, link="logistic"))
        assert np.isnan(pr[17]).all() and (lab[17] == 0).all()  # as NumPy: clip keeps the NaN, NaN > 0 is False


# ----------------------------------------------------------------------------------------------------------------
# links
# ----------------------------------------------------------------------------------------------------------------
LINK_SEEDS = {("f64", "C"): 31, ("f64", "F"): 32, ("f32", "C"): 33, ("f32", "F"): 34}


def _link_problem(dt, layout, R):
    """n = 4097, p = 600, m = 20: eta of standard deviation about 13, so that some rows clip at +-25"""
    rng = np.random.default_rng(LINK_SEEDS[(dt, layout)] + 100 * R)
    n, m = 4097, 20
    vals = rng.standard_normal((n, P)).astype(DT[dt])
    cols, B, c = _model(rng, P, m, R, scales=False)
    B *= 3.0
    return vals, cols, B, c


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("dt,layout", sorted(LINK_SEEDS))
def test_links_against_longdouble(gpu, dt, layout, R):
    vals, cols, B, c = _link_problem(dt, layout, R)
    t = _dev(vals) if layout == "C" else _dev(vals.T).T
    eta, delta = _reference(vals, cols, B, c)
    excluded = int(np.count_nonzero(np.abs(eta) <= delta))
    assert excluded == 0, "seed precondition: %d rows with |eta*| <= Delta" % excluded
    assert (np.abs(eta) > 25).any() and (np.abs(eta) < 25).any()  # both sides of the clip are exercised
    pr, lab = gpu.predict_device(t, cols, B, c, link="logistic")
    e = np.exp(np.clip(eta, LD(-25), LD(25)))
    pr_ref = e / (e + LD(1))
    err = np.abs(_host(pr).astype(LD) - pr_ref)
    bound = delta / LD(4) + LD(8) * U
    print("pr %s %s R=%d: max err %.3e, min slack %.3e" % (dt, layout, R, float(err.max()), float((bound - err).min())))
    assert (err <= bound).all()
    assert np.array_equal(_host(lab), (eta > 0).astype(np.float64))
    lam = gpu.predict_device(t, cols, B, c, link="poisson")
    lam_ref = np.exp(eta)
    rel = np.abs(_host(lam).astype(LD) - lam_ref) / lam_ref
    print("lam %s %s R=%d: max rel err %.3e" % (dt, layout, R, float(rel.max())))
    assert (rel <= delta + LD(8) * U).all()
    for a in (pr, lab, lam):
        assert isinstance(a, torch.Tensor) and tuple(a.shape) == (4097, R) and a.dtype == torch.float64


# ----------------------------------------------------------------------------------------------------------------
# out=
# ----------------------------------------------------------------------------------------------------------------
def test_out_writes_in_place_and_leaves_the_rest_untouched(gpu):
    rng = np.random.default_rng(8)
    n, p, m, R = 1000, 50, 12, 3
    vals = _design(rng, (n, p), np.float64)
    t = _dev(vals)
    cols, B, c = _model(rng, p, m, R)
    want = gpu.predict_device(t, cols, B, c)
    # a dense tensor
    out = torch.full((n, R), -7.0, dtype=torch.float64, device="cuda")
    res = gpu.predict_device(t, cols, B, c, out=out)
    assert res is out and torch.equal(out, want)
    # a column-strided view in the middle of a larger tensor
    big = torch.full((n + 4, 2 * R + 3), -7.0, dtype=torch.float64, device="cuda")
    view = big[2:2 + n, 1:1 + 2 * R:2]
    assert tuple(view.shape) == (n, R) and view.stride() == (2 * R + 3, 2)
    gpu.predict_device(t, cols, B, c, out=view)
    assert torch.equal(view, want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[2:2 + n, 1:1 + 2 * R:2] = False
    assert (big[mask] == -7.0).all()
    # a transposed (column-major) destination, and a vector for one response
    outT = torch.full((R, n), -7.0, dtype=torch.float64, device="cuda")
    gpu.predict_device(t, cols, B, c, out=outT.T)
    assert torch.equal(outT.T, want)
    vec = torch.full((2 * n,), -7.0, dtype=torch.float64, device="cuda")
    gpu.predict_device(t, cols, B[:, 0], c[:1], out=vec[::2])
    assert torch.equal(vec[::2], want[:, 0]) and (vec[1::2] == -7.0).all()
    # the logistic pair
    pr, lab = gpu.predict_device(t, cols, B * 1e-3, c * 1e-3, link="logistic")
    o1, o2 = torch.zeros((n, R), dtype=torch.float64, device="cuda"), torch.zeros((n, R), dtype=torch.float64, device="cuda")
    gpu.predict_device(t, cols, B * 1e-3, c * 1e-3, link="logistic", out=(o1, o2))
    assert torch.equal(o1, pr) and torch.equal(o2, lab)


def test_a_host_pointer_as_device_out_is_an_argument_error(gpu):
    rng = np.random.default_rng(9)
    t = _dev(rng.standard_normal((64, 8)))
    cols = np.array([1, 3], dtype=np.int32)
    B, c, out = np.array([1.0, 2.0]), np.array([0.5]), np.full(64, -7.0)
    lib = gpu.lib()
    rc = lib.bessx_predict_device(t.data_ptr(), 0, 8, 1, 64, 8, gpu._ip(cols), 2, gpu._dp(B), gpu._dp(c), 1, 0,
                                  out.ctypes.data, 1, 1, None, 1, None)
    assert rc == 1 and b"out" in lib.bessx_last_error()  # BESSX_ERR_ARG
    assert (out == -7.0).all()
    # a device view that reaches past its allocation is refused too
    small = torch.zeros(32, dtype=torch.float64, device="cuda")
    rc = lib.bessx_predict_device(t.data_ptr(), 0, 8, 1, 64, 8, gpu._ip(cols), 2, gpu._dp(B), gpu._dp(c), 1, 0,
                                  small.data_ptr(), 1 << 24, 1, None, 1, None)
    assert rc == 1


# ----------------------------------------------------------------------------------------------------------------
# estimators
# ----------------------------------------------------------------------------------------------------------------
def _est_model(est):
    beta = np.asarray(est.beta, dtype=np.float64)
    cols = np.nonzero(beta.any(axis=1) if beta.ndim == 2 else beta)[0]
    return cols, beta[cols], np.asarray(est.coef0, dtype=np.float64).reshape(-1)


def test_lm_estimator_predicts_on_the_device(gpu):
    X, y, _, _ = synth.make_lm(600, 80, 6, seed=71)
    Xd = _dev(X)
    keep = Xd.clone()
    est = linear.PdasLm(sequence=list(range(1, 10)))
    est.fit(Xd, y)
    got = est.predict(Xd)
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (600,)
    host = est.predict(Xd.cpu().numpy())
    eta, delta = _reference(X, *_est_model(est))
    _check_eta(got, eta, delta, "PdasLm")
    assert (np.abs(_host(got).astype(LD) - host.astype(LD)) <= 2 * delta[:, 0]).all()
    assert torch.equal(Xd, keep)
    # a float32 column-major design
    Xf = _dev(X.astype(np.float32).T).T
    got32 = est.predict(Xf)
    eta32, delta32 = _reference(X.astype(np.float32), *_est_model(est))
    _check_eta(got32, eta32, delta32, "PdasLm fp32 column-major")


def test_multi_response_lm_returns_n_by_r(gpu):
    X, y, _, _ = synth.make_lm(600, 80, 6, seed=72)
    rng = np.random.default_rng(73)
    Y = np.column_stack([y, X[:, 3] - 2 * X[:, 11] + 0.1 * rng.standard_normal(600), rng.standard_normal(600)])
    Xd = _dev(X)
    est = linear.PdasLm(sequence=list(range(1, 8)))
    est.fit(Xd, Y)
    assert est.beta.shape == (80, 3)
    got = est.predict(Xd)
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (600, 3)
    host = est.predict(X)
    eta, delta = _reference(X, *_est_model(est))
    _check_eta(got, eta, delta, "multi-response PdasLm")
    assert (np.abs(_host(got).astype(LD) - host.astype(LD)) <= 2 * delta).all()


def test_logistic_and_poisson_estimators_predict_on_the_device(gpu):
    X, y, _, _ = synth.make_logistic(1500, 40, 4, seed=74)
    Xd = _dev(X)
    est = linear.PdasLogistic(sequence=list(range(1, 7)))
    est.fit(Xd, y)
    got = est.predict(Xd)
    assert sorted(got) == ["Y", "pr"] and all(isinstance(v, torch.Tensor) and v.is_cuda and tuple(v.shape) == (1500,)
                                              for v in got.values())
    host = est.predict(X)
    eta, delta = _reference(X, *_est_model(est))
    assert not (np.abs(eta) <= delta).any()
    assert np.array_equal(_host(got["Y"]), host["Y"]) and np.array_equal(host["Y"], (eta[:, 0] > 0).astype(float))
    bound = delta[:, 0] / LD(4) + LD(8) * U
    assert (np.abs(_host(got["pr"]).astype(LD) - host["pr"].astype(LD)) <= 2 * bound).all()

    X, y, _, _ = synth.make_poisson(1500, 40, 4, seed=75)
    Xd = _dev(X)
    est = linear.PdasPoisson(sequence=list(range(1, 7)))
    est.fit(Xd, y)
    got = est.predict(Xd)
    assert list(got) == ["lam"] and isinstance(got["lam"], torch.Tensor) and tuple(got["lam"].shape) == (1500,)
    host = est.predict(X)
    eta, delta = _reference(X, *_est_model(est))
    lam_ref = np.exp(eta[:, 0])
    rel = np.abs(_host(got["lam"]).astype(LD) - host["lam"].astype(LD)) / lam_ref
    assert (rel <= 2 * (delta[:, 0] + LD(8) * U)).all()


def test_cox_estimator_returns_none_for_a_device_x(gpu):
    X, obs, status, _, _ = synth.make_cox(400, 30, 3, seed=76)
    Xd = _dev(X)
    est = linear.PdasCox(sequence=[1, 2, 3])
    est.fit(Xd, np.column_stack([obs, status]))
    assert est.predict(Xd) is None
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 30"):
        est.predict(Xd[:, :29])


def test_x_written_on_a_side_stream_just_before_the_call_is_read_after_it(gpu):
    X, y, _, _ = synth.make_lm(4000, 300, 10, seed=77)
    est = linear.PdasLm(sequence=list(range(1, 13)))
    src = _dev(X)
    est.fit(src, y)
    want = est.predict(src)
    Xd = torch.zeros_like(src)
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(40):  # tens of milliseconds of work in front of the copy
            a = a @ a
            a = a / a.abs().max()
        Xd.copy_(src)
        got = est.predict(Xd)  # (torch's current stream is `side`)
    assert np.array_equal(_bits(got), _bits(want))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------
# full size
# ----------------------------------------------------------------------------------------------------------------
def test_full_size_row_major_and_column_major(gpu):
    """configs[1] (n = 50 000, p = 10 000, fp64: 4 GB, byte offsets beyond 2^32), m = 200, 2 000 sampled rows."""
    n, p, m, R = 50000, 10000, 200, 2
    g = torch.Generator(device="cuda").manual_seed(7)
    big = torch.randn((n, p), generator=g, device="cuda", dtype=torch.float64)
    rng = np.random.default_rng(78)
    cols, B, c = _model(rng, p, m, R)
    rows = np.sort(rng.choice(n, 2000, replace=False))
    rows[-1] = n - 1
    for name, t in (("row-major", big), ("column-major", big.view(p, n).T)):
        assert tuple(t.shape) == (n, p)
        vals = t[torch.from_numpy(rows).cuda()][:, torch.from_numpy(cols.astype(np.int64)).cuda()].cpu().numpy()
        eta, delta = _reference(vals, np.arange(m), B, c)
        got = gpu.predict_device(t, cols, B, c)
        assert tuple(got.shape) == (n, R)
        _check_eta(_host(got)[rows], eta, delta, "full size " + name)
    del big
