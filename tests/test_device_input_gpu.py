"""X already in GPU memory (bessx_session_create_device, bess_amd/csrc/bessx_k_ingest.hip): the ingest kernel leaves in the
session bit for bit what the host upload leaves for the same values, and everything after it is the same deterministic
code -- so every comparison here is exact (np.array_equal): the kernel against NumPy's padded column-major image, device
sessions and estimators against their host twins."""
import ctypes

import numpy as np
import pytest

from bess_amd import linear, synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DT = {"f64": (np.float64, torch.float64), "f32": (np.float32, torch.float32)}
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 65), (1000, 37), (4097, 130)]
LAYOUTS = ["C", "F", "T", "colslice_odd", "rows2", "cols3"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _view(layout, n, p, npdt, rng):
    """(base host array, function base tensor -> the n x p view under test, the view's values on the host)"""
    if layout == "C":
        b = rng.standard_normal((n, p)).astype(npdt)
        return b, (lambda t: t), b
    if layout == "F":  # column-contiguous: the transpose of a C-contiguous p x n tensor
        b = rng.standard_normal((p, n)).astype(npdt)
        return b, (lambda t: t.T), b.T
    if layout == "T":  # .T of an F-ordered thing = row-contiguous again, through two views
        b = rng.standard_normal((n, p)).astype(npdt)
        return b, (lambda t: t.T.T), b
    if layout == "colslice_odd":  # columns 3 .. 3+p of a wider tensor: an odd first element
        b = rng.standard_normal((n, p + 5)).astype(npdt)
        return b, (lambda t: t[:, 3:3 + p]), b[:, 3:3 + p]
    if layout == "rows2":
        b = rng.standard_normal((2 * n, p)).astype(npdt)
        return b, (lambda t: t[::2]), b[::2]
    if layout == "cols3":
        b = rng.standard_normal((n, 3 * p)).astype(npdt)
        return b, (lambda t: t[:, ::3]), b[:, ::3]
    raise AssertionError(layout)


def _image(vals, ld):
    img = np.zeros((ld, vals.shape[1]), order="F")
    img[:vals.shape[0]] = vals.astype(np.float64)
    return img


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ingest_kernel_matches_numpy_image(gpu, dt, layout):
    npdt, _ = DT[dt]
    rng = np.random.default_rng(11)
    for n, p in SHAPES:
        base, view, vals = _view(layout, n, p, npdt, rng)
        tb = _dev(base)
        t = view(tb)
        assert tuple(t.shape) == (n, p)
        ld = gpu.padded_rows(n)
        for order in (None, rng.permutation(n).astype(np.int32)):
            got, nan = gpu.op_ingest(t, row_order=order)
            want = _image(vals if order is None else vals[order], ld)
            assert got.shape == (ld, p)
            assert np.array_equal(got, want), (dt, layout, n, p, order is not None)
            assert not got[n:].any()  # padding rows are zeros
            assert nan is False
        assert np.array_equal(tb.cpu().numpy(), base)  # the source is never written
        # a single NaN in the last row and last column raises the flag
        tb2 = tb.clone()
        view(tb2)[n - 1, p - 1] = float("nan")
        _, nan = gpu.op_ingest(view(tb2))
        assert nan is True


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_ingest_column_contiguous_aligned_and_odd_bases(gpu, dt):
    """Column-contiguous sources: the 16-byte path (aligned base and column stride) and the element path (a row offset
    that leaves the base on an odd element, an odd column stride)."""
    npdt, _ = DT[dt]
    rng = np.random.default_rng(12)
    for n, p, cs, off in [(1000, 37, 1000, 0), (1000, 37, 1001, 0), (1000, 37, 1004, 1), (4097, 130, 4100, 3),
                          (4097, 130, 4100, 0)]:
        base = rng.standard_normal((p, cs)).astype(npdt)
        tb = _dev(base)
        t = tb[:, off:off + n].T
        got, nan = gpu.op_ingest(t)
        assert np.array_equal(got, _image(base[:, off:off + n].T, gpu.padded_rows(n))) and not nan


def test_ingest_indexes_in_64_bits(gpu):
    """A 64-column slice at the far end of one fp32 tensor of more than 2^31 elements (allocated, never filled)."""
    n, ptot, p = 8192, 262400, 64
    need = n * ptot * 4
    free, _ = torch.cuda.mem_get_info()
    if free < need + (1 << 30):
        pytest.skip("needs %.1f GB of free device memory" % (need / 1e9))
    big = torch.empty((n, ptot), dtype=torch.float32, device="cuda")
    assert big.numel() > 2 ** 31
    sl = big[:, ptot - p:]
    g = torch.Generator(device="cuda").manual_seed(5)
    sl.copy_(torch.randn((n, p), generator=g, device="cuda", dtype=torch.float32))
    got, nan = gpu.op_ingest(sl)
    assert np.array_equal(got[:n], sl.cpu().numpy().astype(np.float64)) and not nan
    # ... and with a row order (rows reversed)
    order = np.arange(n - 1, -1, -1).astype(np.int32)
    got2, _ = gpu.op_ingest(sl, row_order=order)
    assert np.array_equal(got2[:n], sl.cpu().numpy().astype(np.float64)[::-1])
    del big, sl


# ----------------------------------------------------------------------------------------------------------------
# sessions
# ----------------------------------------------------------------------------------------------------------------
def _same_result(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        if k in ("device_seconds", "trace"):
            continue
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


def _cox_sorted(n, p, k, seed):
    X, _, status, _, _ = synth.make_cox(n, p, k, seed=seed)  # (rows come sorted by time)
    return X, status


def _family(name):
    if name in ("lm", "lm_stream"):
        X, y, _, _ = synth.make_lm(600, 120, 6, seed=21)
        kw = dict(model_type=1, data_type=1, score_mode=1 if name == "lm_stream" else 2)
    elif name == "logistic":
        X, y, _, _ = synth.make_logistic(600, 80, 5, seed=22)
        kw = dict(model_type=2, data_type=2)
    elif name == "poisson":
        X, y, _, _ = synth.make_poisson(600, 80, 5, seed=23)
        kw = dict(model_type=3, data_type=2)
    else:
        X, y = _cox_sorted(500, 60, 5, 24)
        kw = dict(model_type=4, data_type=3)
    return X, np.asarray(y, dtype=np.float64), kw


FAMILIES = ["lm", "lm_stream", "logistic", "poisson", "cox"]


@pytest.mark.parametrize("fam", FAMILIES)
def test_device_session_paths_equal_host_session(gpu, fam):
    X, y, kw = _family(fam)
    n, p = X.shape
    Xd = _dev(X)
    seq = np.arange(1, 9)
    folds = synth.make_cv_folds(n, 4)
    with gpu.Session(X, y, **kw) as h, gpu.Session(Xd, y, **kw) as d:
        c = d.counters()
        assert c["x_bytes_uploaded_from_host"] == 0 and c["x_bytes_ingested_on_device"] == n * p * 8
        ch = h.counters()
        assert ch["x_bytes_uploaded_from_host"] == n * p * 8 and ch["x_bytes_ingested_on_device"] == 0
        for u, v in zip(h.normalization(), d.normalization()):
            assert np.array_equal(u, v)
        lam = (0.0, 0.05) if fam.startswith("lm") else (0.0,)
        _same_result(h.sequential_path(seq, lam, ic_type=3), d.sequential_path(seq, lam, ic_type=3), fam + " seq")
        _same_result(h.gs_path(1, 12, ic_type=3), d.gs_path(1, 12, ic_type=3), fam + " gs")
        h.set_cv(4, folds)
        d.set_cv(4, folds)
        _same_result(h.sequential_path(seq[:5], (0.0,), ic_type=3, is_cv=True),
                     d.sequential_path(seq[:5], (0.0,), ic_type=3, is_cv=True), fam + " cv")
    kw5 = dict(kw, algorithm_type=5)
    with gpu.Session(X, y, **kw5) as h, gpu.Session(Xd, y, **kw5) as d:
        _same_result(h.pgs_path(1, 8, 0.01, 1.0, n_lambda=5, ic_type=3), d.pgs_path(1, 8, 0.01, 1.0, n_lambda=5, ic_type=3),
                     fam + " pgs")


@pytest.mark.parametrize("fam", ["lm", "logistic", "cox"])
def test_device_session_fp32_weights_and_device_y(gpu, fam):
    """fp32 device X equals the host session on X.astype(float64); y and weight as device vectors (fp32 y for LM)."""
    X, y, kw = _family(fam)
    n, p = X.shape
    X32 = X.astype(np.float32)
    w = np.random.default_rng(3).uniform(0.5, 1.5, n)
    yd = _dev(y.astype(np.float32)) if fam == "lm" else _dev(y)
    yh = y.astype(np.float32).astype(np.float64) if fam == "lm" else y
    seq = np.arange(1, 8)
    with gpu.Session(X32.astype(np.float64), yh, weight=w, **kw) as h, \
            gpu.Session(_dev(X32), yd, weight=_dev(w), **kw) as d:
        assert d.counters()["x_bytes_ingested_on_device"] == n * p * 4
        assert d.counters()["x_bytes_uploaded_from_host"] == 0
        for u, v in zip(h.normalization(), d.normalization()):
            assert np.array_equal(u, v)
        _same_result(h.sequential_path(seq, ic_type=3), d.sequential_path(seq, ic_type=3), fam + " fp32")


def test_device_session_groups_and_strided_views(gpu):
    X, y, _, _ = synth.make_lm(500, 96, 6, seed=31)
    gi = np.arange(0, 96, 4)
    seq = np.arange(1, 6)
    wide = _dev(np.concatenate([np.zeros((500, 3)), X, np.ones((500, 2))], axis=1))
    views = {"C": _dev(X), "F": _dev(X.T).T, "slice": wide[:, 3:99], "rows2": _dev(np.repeat(X, 2, axis=0))[::2]}
    with gpu.Session(X, y, g_index=gi, algorithm_type=2) as h:
        want = h.sequential_path(seq, ic_type=3)
    for name, v in views.items():
        with gpu.Session(v, y, g_index=gi, algorithm_type=2) as d:
            _same_result(want, d.sequential_path(seq, ic_type=3), "groups " + name)


@pytest.mark.parametrize("fam", ["lm", "logistic", "cox"])
def test_device_session_screening(gpu, fam):
    X, y, kw = _family(fam)
    p = X.shape[1]
    seq = np.arange(1, 6)
    kws = dict(kw, is_screening=True, screening_size=20)
    with gpu.Session(X, y, **kws) as h, gpu.Session(_dev(X), y, **kws) as d:
        assert np.array_equal(h.screening(), d.screening())
        assert d.counters()["x_bytes_uploaded_from_host"] == 0
        _same_result(h.sequential_path(seq, ic_type=3), d.sequential_path(seq, ic_type=3), fam + " screening")
    # groups: width 4 everywhere, and for the logistic model one group of 12 columns (wider than the register-resident
    # marginal fit: a sub-session on a column-offset view of the device matrix)
    gi = np.arange(0, p, 4)
    if fam == "logistic":
        gi = np.concatenate([[0], np.arange(12, p, 4)])
    alg = 2
    kwg = dict(kw, is_screening=True, screening_size=8, g_index=gi, algorithm_type=alg)
    with gpu.Session(X, y, **kwg) as h, gpu.Session(_dev(X), y, **kwg) as d, \
            gpu.Session(_dev(X.T).T, y, **kwg) as f:
        for o in (d, f):
            assert np.array_equal(h.screening(), o.screening())
            assert np.array_equal(h.screening_groups(), o.screening_groups())
            _same_result(h.sequential_path(seq[:3], ic_type=3), o.sequential_path(seq[:3], ic_type=3), fam + " group scr")


def test_device_responses(gpu):
    X, y, _, _ = synth.make_lm(800, 150, 6, seed=41)
    rng = np.random.default_rng(42)
    Y = np.stack([y, X[:, :5] @ rng.standard_normal(5) + 0.1 * rng.standard_normal(800),
                  X[:, 10:14] @ rng.standard_normal(4) + 0.1 * rng.standard_normal(800)], axis=1)
    seq = np.arange(1, 10)
    with gpu.Session(X, y) as h, gpu.Session(_dev(X), _dev(y)) as d:
        h.set_responses(Y)
        want = h.sequential_path_multi(seq, ic_type=3)
        for Yd in (_dev(Y), _dev(Y.T).T, _dev(np.repeat(Y, 2, axis=1))[:, ::2]):
            d.set_responses(Yd)
            got = d.sequential_path_multi(seq, ic_type=3)
            assert len(got) == len(want) == 3
            for r in range(3):
                _same_result(want[r], got[r], "response %d" % r)
    Y32 = Y.astype(np.float32)
    with gpu.Session(X, y) as h, gpu.Session(_dev(X), y) as d:
        h.set_responses(Y32.astype(np.float64))
        d.set_responses(_dev(Y32))
        for a, b in zip(h.sequential_path_multi(seq, ic_type=3), d.sequential_path_multi(seq, ic_type=3)):
            _same_result(a, b, "fp32 responses")


def test_source_may_be_overwritten_after_the_constructor(gpu):
    X, y, _, _ = synth.make_lm(700, 100, 5, seed=51)
    seq = np.arange(1, 8)
    with gpu.Session(X, y, score_mode=1) as h:
        want = h.sequential_path(seq, ic_type=3)
    Xd = _dev(X)
    with gpu.Session(Xd, y, score_mode=1) as d:
        Xd.zero_()
        torch.cuda.synchronize()
        _same_result(want, d.sequential_path(seq, ic_type=3), "overwritten source")


def test_reads_are_ordered_after_the_callers_stream(gpu):
    """X is produced on a side stream behind a long-running kernel; the stream is passed, nothing is synchronised."""
    X, y, _, _ = synth.make_lm(700, 100, 5, seed=52)
    seq = np.arange(1, 8)
    with gpu.Session(X, y) as h:
        want = h.sequential_path(seq, ic_type=3)
    src = _dev(X)
    Xd = torch.zeros_like(src)
    a = torch.randn((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(40):  # tens of milliseconds of work in front of the copy
            a = a @ a
            a = a / a.abs().max()
        Xd.copy_(src)
    with gpu.Session(Xd, y, stream=side.cuda_stream) as d:
        _same_result(want, d.sequential_path(seq, ic_type=3), "side stream")
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------
# estimators
# ----------------------------------------------------------------------------------------------------------------
def _same_fit(a, b, what):
    for k in ("beta", "coef0", "train_loss", "ic"):
        assert np.array_equal(np.asarray(getattr(a, k)), np.asarray(getattr(b, k))), (what, k)


def test_estimators_on_device_x(gpu):
    Xl, yl, _, _ = synth.make_lm(600, 100, 5, seed=61)
    Xg, yg, _, _ = synth.make_logistic(600, 60, 4, seed=62)
    Xp, yp, _, _ = synth.make_poisson(600, 60, 4, seed=63)
    Xc, tc, sc, _, _ = synth.make_cox(500, 50, 4, seed=64)
    shuffle = np.random.default_rng(65).permutation(500)
    Xc, yc = np.ascontiguousarray(Xc[shuffle]), np.stack([tc[shuffle], sc[shuffle]], axis=1)
    assert (np.diff(yc[:, 0]) < 0).any()  # unsorted times: the device fit sorts through row_order
    seq = list(range(1, 9))
    cases = [
        ("PdasLm", lambda: linear.PdasLm(sequence=seq), Xl, yl, {}),
        ("PdasLm cv", lambda: linear.PdasLm(sequence=seq, is_cv=True, K=4), Xl, yl, {}),
        ("PdasLm gs", lambda: linear.PdasLm(path_type="pgs", s_min=1, s_max=12), Xl, yl, {}),
        ("PdasLm screening", lambda: linear.PdasLm(sequence=seq, is_screening=True, screening_size=30), Xl, yl, {}),
        ("PdasLm always", lambda: linear.PdasLm(sequence=seq, always_select=[2, 7]), Xl, yl, {}),
        ("PdasLm weight", lambda: linear.PdasLm(sequence=seq), Xl, yl,
         dict(is_weight=True, weight=np.random.default_rng(7).uniform(0.5, 2.0, 600))),
        ("PdasLogistic", lambda: linear.PdasLogistic(sequence=seq), Xg, yg, {}),
        ("PdasPoisson", lambda: linear.PdasPoisson(sequence=seq), Xp, yp, {}),
        ("PdasCox", lambda: linear.PdasCox(sequence=seq), Xc, yc, {}),
        ("GroupPdasLm", lambda: linear.GroupPdasLm(sequence=seq[:5]), Xl, yl, dict(group=np.repeat(np.arange(25), 4))),
        ("L0L2Lm", lambda: linear.L0L2Lm(sequence=seq, lambda_sequence=[0.0, 0.1, 1.0]), Xl, yl, {}),
        ("L0L2Lm pgs", lambda: linear.L0L2Lm(path_type="pgs", s_min=1, s_max=8, lambda_min=0.01, lambda_max=1.0), Xl, yl, {}),
    ]
    for what, make, X, y, kw in cases:
        h, d = make(), make()
        h.fit(X, y, **kw)
        d.fit(_dev(X), y, **kw)
        _same_fit(h, d, what)
    # fp32 device X = the host fit on the widened values; y on the device too
    h, d = linear.PdasLm(sequence=seq), linear.PdasLm(sequence=seq)
    h.fit(Xl.astype(np.float32).astype(np.float64), yl)
    d.fit(_dev(Xl.astype(np.float32)), _dev(yl))
    _same_fit(h, d, "fp32")


def test_estimator_with_2d_device_response(gpu):
    X, y, _, _ = synth.make_lm(600, 100, 5, seed=71)
    rng = np.random.default_rng(72)
    Y = np.stack([y, X[:, 3:7] @ rng.standard_normal(4) + 0.1 * rng.standard_normal(600)], axis=1)
    h, d = linear.PdasLm(sequence=list(range(1, 8))), linear.PdasLm(sequence=list(range(1, 8)))
    h.fit(X, Y)
    d.fit(_dev(X), _dev(Y))
    assert d.beta.shape == (100, 2)
    _same_fit(h, d, "2-D device y")


def test_nan_in_device_x_raises_the_estimators_message(gpu):
    X, y, _, _ = synth.make_lm(300, 40, 3, seed=81)
    X[299, 39] = np.nan
    with pytest.raises(ValueError, match="There is NAN value in X"):
        linear.PdasLm(sequence=[1, 2, 3]).fit(_dev(X), y)
    with pytest.raises(ValueError, match="There is NAN value in X"):
        gpu.Session(_dev(X), y)


def test_host_pointers_are_refused_cleanly(gpu):
    """A host pointer in the descriptor is BESSX_ERR_ARG with a message, not a fault (and so is memory of another
    device, when there is one)."""
    lib = gpu.lib()
    X, y, _, _ = synth.make_lm(200, 30, 3, seed=91)
    X = np.ascontiguousarray(X)
    y = np.ascontiguousarray(y)

    def create(xptr, device=-1, ydev=None):
        pb = gpu.Problem(200, 30, None, 0, None, None, 1, 1, 1, 1, 20, 1, None, 0, device, None, 0, 0, 0, 0, 0)
        din = gpu.DeviceInput()
        din.x, din.x_dtype, din.x_row_stride, din.x_col_stride = xptr, 0, 30, 1
        if ydev is None:
            din.y_host = y.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        else:
            din.y_dev, din.y_dtype, din.y_stride = ydev, 0, 1
        h = ctypes.c_void_p()
        rc = lib.bessx_session_create_device(ctypes.byref(h), ctypes.byref(pb), ctypes.byref(din))
        if rc == 0:
            lib.bessx_session_destroy(h)
        return rc, gpu.last_error()

    rc, msg = create(X.ctypes.data)
    assert rc == 1 and "device" in msg, (rc, msg)
    Xd = _dev(X)
    rc, msg = create(Xd.data_ptr(), ydev=y.ctypes.data)  # y_dev pointing at host memory
    assert rc == 1 and "device input y" in msg, (rc, msg)
    rc, msg = create(Xd.data_ptr())
    assert rc == 0, msg
    if torch.cuda.device_count() > 1:
        other = torch.zeros((200, 30), dtype=torch.float64, device="cuda:1")
        rc, msg = create(other.data_ptr(), device=0)
        assert rc == 1 and "another device" in msg, (rc, msg)
        rc, msg = create(Xd.data_ptr(), ydev=other.data_ptr())
        assert rc == 1 and "another device" in msg, (rc, msg)
