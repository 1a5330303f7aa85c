"""Row diagnostics on an X already in GPU memory (bessx_diag_device, bess_amd/csrc/bessx_k_diag.hip) against NumPy in
np.longdouble on the host copy of the same values, within the bounds derived in tests/diagref.py.  Shapes: n = 1, 15,
16, 17 around the 16-row tile of the matrix-core kernel, 127 a partial last tile, 4097 many tiles; m + 1 = 1, 2, 15, 16,
17 around one output tile, 32 = two tiles, 201 = thirteen with a ragged last one, 1024 the largest, 1025 refused.
Layouts and the NaN embedding are those of tests/test_info_gpu.py, every element outside the view a NaN.  The design
of n rows is the first n rows of that file's 4097-row problem, and the factor R comes from the information of all 4097
rows (fp64 NumPy, capi.info_factor) for the same link and weights: every row is then in the sample and its leverage
lies below 1, whatever n is -- the kernel does not care where R came from."""
import numpy as np
import pytest

import diagref
import inforef
from bess_amd import linear
from test_info_gpu import DT, LAYOUTS, LINKS, P, _dev, _embed, _forms, _problem

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
NB = 4097
NS, MS = (1, 15, 16, 17, 127, 4097), (0, 1, 14, 15, 16, 31, 200)
KINDS = diagref.KINDS

_SUB, _FACTORS, _GEOM, _REFS = {}, {}, {}, {}


def _sub(dt, n, m, p=P):
    """The first n rows of the 4097-row problem of (dt, m): the same logical values under every layout."""
    key = (dt, n, m, p)
    if key not in _SUB:
        pr = _problem(dt, NB, m, p)
        _SUB[key] = dict(vals=pr["vals"][:n], cols=pr["cols"], beta=pr["beta"], c=pr["c"],
                         ys={k: v[:n] for k, v in pr["ys"].items()}, w=pr["w"][:n])
    return _SUB[key]


def _factor(dt, m, p=P):
    """R of (dt, m): the factor of the weighted Poisson information of all 4097 rows (fp64 NumPy, capi.info_factor).  Of
    the three links' working weights the Poisson ones are the largest, so with this R every link's leverages lie
    below 1 (the reference asserts it)."""
    key = (dt, m, p)
    if key not in _FACTORS:
        pr = _problem(dt, NB, m, p)
        got = linear.bess_base._information_host("poisson", pr["vals"][:, pr["cols"]].astype(np.float64), pr["beta"],
                                                 pr["c"], pr["ys"]["poisson"], pr["w"])
        R, pd = linear.capi.info_factor(got["info"])
        assert pd
        _FACTORS[key] = R
    return _FACTORS[key]


def _phi(dt, m, link, p=P):
    """The dispersion as bess_base.diagnostics takes it: the weighted residual variance of the 4097 rows for the identity
    link (any positive number would do for the kernel), 1 otherwise."""
    if link != "identity":
        return 1.0
    pr = _problem(dt, NB, m, p)
    e = pr["ys"][link] - (pr["vals"][:, pr["cols"]].astype(np.float64) @ pr["beta"] + pr["c"])
    return float((pr["w"] * e * e).sum() / (pr["w"].sum() - (m + 1)))


def _ref(dt, n, m, link, y32, weighted, p=P):
    """diagref.diagnostics_reference at the device's addition depth, once per distinct set of values; the links,
    responses and weights of one (dt, n, m) share the longdouble product Z R^T"""
    key = (dt, n, m, link, y32, weighted, p)
    if key not in _REFS:
        pr = _sub(dt, n, m, p)
        R = _factor(dt, m, p)
        if (dt, n, m, p) not in _GEOM:
            _GEOM[(dt, n, m, p)] = diagref.geometry(pr["vals"], pr["cols"], R)
        y = pr["ys"][link].astype(np.float32) if y32 else pr["ys"][link]
        _REFS[key] = diagref.diagnostics_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], y,
                                                   pr["w"] if weighted else None, link, R, _phi(dt, m, link, p),
                                                   diagref.sum_depth(m + 1), geom=_GEOM[(dt, n, m, p)])
    return _REFS[key]


def _np(got):
    return {k: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for k, v in got.items()}


def _run(gpu, t, pr, link, y, w, R, phi, **kw):
    return _np(gpu.diagnostics_device(t, pr["cols"], pr["beta"], pr["c"], y, factor=R, dispersion=phi, link=link,
                                      weight=w, **kw))


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a) and set(a) == set(b)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_all_seven_kinds_are_within_the_bounds(gpu, dt, layout, n):
    base, view = _embed(layout, _problem(dt, NB, 0)["vals"][:n])
    t = view(_dev(base))
    assert tuple(t.shape) == (n, P)
    ni = NS.index(n)
    for mi, m in enumerate(MS):
        pr = _sub(dt, n, m)
        for li, link in enumerate(LINKS):
            fi, wi = (mi + li) % 4, (mi + 2 * li + ni) % 5
            y, w, y32 = _forms(pr, link, fi, wi)
            R, phi = _factor(dt, m), _phi(dt, m, link)
            ref = _ref(dt, n, m, link, y32, wi > 0)
            got = gpu.diagnostics_device(t, pr["cols"], pr["beta"], pr["c"], y, factor=R, dispersion=phi, link=link,
                                         weight=w)
            assert list(got) == list(KINDS)
            for k in KINDS:  # views of ONE (7, n) tensor on x's device
                assert got[k].shape == (n,) and got[k].device == t.device and got[k].dtype == torch.float64
                assert got[k].data_ptr() == got["leverage"].data_ptr() + 8 * n * KINDS.index(k)
            got = _np(got)
            diagref.check_diagnostics(got, ref, "%s %s n=%d m=%d %s y%d w%d" % (dt, layout, n, m, link, fi, wi))
            if wi > 0:
                zero = pr["w"] == 0
                for k in ("leverage", "pearson", "deviance", "std_pearson", "std_deviance", "cooks"):
                    assert (got[k][zero] == 0).all(), k


@pytest.mark.parametrize("layout", ["C", "F"])
def test_the_largest_support_and_one_past_it(gpu, layout):
    n, p, m = 127, 1100, 1023
    pr = _sub("f64", n, m, p)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    R, phi = _factor("f64", m, p), 1.0
    ref = _ref("f64", n, m, "logistic", False, True, p)
    got = _run(gpu, t, pr, "logistic", pr["ys"]["logistic"], pr["w"], R, phi)
    diagref.check_diagnostics(got, ref, "m + 1 = 1024 " + layout)
    with pytest.raises(gpu.BessxError) as e:
        gpu.diagnostics_device(t, np.arange(1024), np.zeros(1024), 0.0, pr["ys"]["logistic"], factor=np.eye(1025),
                               link="logistic")
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_the_five_layouts_give_the_same_bits(gpu, dt):
    n = NB
    first = {}
    for layout in LAYOUTS:
        base, view = _embed(layout, _problem(dt, NB, 0)["vals"])
        t = view(_dev(base))
        for mi, m in enumerate(MS):
            pr = _sub(dt, n, m)
            link = LINKS[mi % 3]
            R, phi = _factor(dt, m), _phi(dt, m, link)
            got = _run(gpu, t, pr, link, pr["ys"][link], pr["w"], R, phi)
            if layout == LAYOUTS[0]:
                first[m] = got
                diagref.check_diagnostics(got, _ref(dt, n, m, link, False, True), "%s m=%d %s" % (dt, m, link))
            else:
                assert _same_bits(first[m], got), (dt, layout, m, link)
        del t


@pytest.mark.parametrize("layout", ["C", "F", "two_strides"])
def test_a_rows_numbers_depend_on_that_row_alone(gpu, layout):
    """A row permutation of X, y and w permutes every output bit for bit; the first 17 rows of the n = 4097 call equal
    the n = 17 call bit for bit; the same call twice gives the same bits."""
    m = 200
    for dt, link in (("f64", "poisson"), ("f32", "logistic")):
        pr = _sub(dt, NB, m)
        R, phi = _factor(dt, m), _phi(dt, m, link)
        y, w = pr["ys"][link], pr["w"]
        base, view = _embed(layout, pr["vals"])
        t = view(_dev(base))
        a = _run(gpu, t, pr, link, _dev(y), _dev(w), R, phi)
        b = _run(gpu, t, pr, link, _dev(y), _dev(w), R, phi)
        assert _same_bits(a, b)
        perm = np.random.default_rng(9).permutation(NB)
        base, view = _embed(layout, pr["vals"][perm])
        c = _run(gpu, view(_dev(base)), pr, link, y[perm], _dev(w[perm]), R, phi)
        assert _same_bits({k: v[perm] for k, v in a.items()}, c), (dt, layout, "permutation")
        base, view = _embed(layout, pr["vals"][:17])
        d = _run(gpu, view(_dev(base)), pr, link, y[:17], w[:17], R, phi)
        assert _same_bits({k: v[:17] for k, v in a.items()}, d), (dt, layout, "first 17 rows")


@pytest.mark.parametrize("layout", ["C", "F"])
def test_residual_kinds_alone_need_no_factor_and_give_the_same_bits(gpu, layout):
    n, m = 4097, 31
    pr = _sub("f64", n, m)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    for link in LINKS:
        R, phi = _factor("f64", m), _phi("f64", m, link)
        full = _run(gpu, t, pr, link, pr["ys"][link], pr["w"], R, phi)
        res = _run(gpu, t, pr, link, pr["ys"][link], pr["w"], None, float("nan"), kinds=["deviance", "response", "pearson"])
        assert list(res) == ["response", "pearson", "deviance"]
        assert _same_bits(res, {k: full[k] for k in res}), link
        # ... and a derived kind alone (its residual goes through workspace) equals the full call's
        for kinds in (["cooks"], ["std_deviance", "leverage"], ["std_pearson"]):
            part = _run(gpu, t, pr, link, pr["ys"][link], pr["w"], R, phi, kinds=kinds)
            assert _same_bits(part, {k: full[k] for k in part}), (link, kinds)


def test_out_with_a_padded_leading_dimension_leaves_the_padding_untouched(gpu):
    n, m = 127, 16
    pr = _sub("f64", n, m)
    t = _dev(pr["vals"])
    R, phi = _factor("f64", m), 1.0
    want = _run(gpu, t, pr, "poisson", pr["ys"]["poisson"], pr["w"], R, phi)
    buf = torch.full((7, n + 9), -7.25, dtype=torch.float64, device=t.device)
    got = gpu.diagnostics_device(t, pr["cols"], pr["beta"], pr["c"], pr["ys"]["poisson"], factor=R, dispersion=phi,
                                 link="poisson", weight=pr["w"], out=buf[:, :n])
    assert _same_bits(_np(got), want)
    h = buf.cpu().numpy()
    assert (h[:, n:] == -7.25).all()
    for s, k in enumerate(KINDS):
        assert np.array_equal(h[s, :n], want[k])
    buf2 = torch.full((2, n + 1), -7.25, dtype=torch.float64, device=t.device)
    gpu.diagnostics_device(t, pr["cols"], pr["beta"], pr["c"], pr["ys"]["poisson"], factor=R, dispersion=phi,
                           link="poisson", weight=pr["w"], kinds=["cooks", "response"], out=buf2[:, :n])
    h = buf2.cpu().numpy()
    assert (h[:, n:] == -7.25).all() and np.array_equal(h[0, :n], want["response"]) and np.array_equal(h[1, :n], want["cooks"])


def test_the_leverages_add_up_to_the_number_of_coefficients(gpu):
    """sum_i h_i = trace(R I R^T) = M up to the error of the factor, which comes from the same 4097 rows: within the sum
    of the leverage bounds plus 2 M rel, rel the relative figure of inforef.se_reference (the derivation is in
    tests/test_diag_api.py)."""
    n, m, link = NB, 31, "poisson"  # (the link and the weights R was made from)
    pr = _sub("f64", n, m)
    R, phi = _factor("f64", m), _phi("f64", m, link)
    got = _run(gpu, _dev(pr["vals"]), pr, link, pr["ys"][link], pr["w"], R, phi, kinds=["leverage"])
    ref = _ref("f64", n, m, link, False, True)
    iref = inforef.information_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], pr["ys"][link], pr["w"], link, n)
    _, _, rel, cond = inforef.se_reference(iref)
    h = got["leverage"].astype(LD)
    bound = ref["h_sum_bound"] + LD(2 * (m + 1)) * rel
    print("sum h - M = %.3e against bound %.3e (cond(S*) %.3e), max h %.4f" % (float(h.sum() - (m + 1)), float(bound),
                                                                             cond, float(h.max())))
    assert abs(h.sum() - LD(m + 1)) <= bound
    assert (h >= 0).all() and (h <= LD(1) + LD(2) * rel + ref["bound"]["leverage"]).all()


@pytest.mark.parametrize("name", ["PdasLm", "PdasLogistic", "PdasPoisson"])
def test_estimator_diagnostics_on_a_device_matrix_agree_with_the_numpy_route(gpu, name):
    """The two routes use their own information matrix, factor and dispersion.  Both factors invert a matrix within
    eps of S* (inforef step 5), so z^T R^T R z of either lies within 2 rel of the exact inverse's and within 4 rel of the
    other's; both dispersions lie within loss_bound / loss* of the exact one.  The reference takes the NumPy route's R
    and phi and carries these two terms in its bounds; the routes then agree within twice the bound."""
    n, p, k = 400, 60, 4
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, p))
    truth = np.zeros(p)
    truth[rng.choice(p, k, replace=False)] = np.array([1.0, -1.0, 0.8, -0.8])
    eta = X @ truth + 0.2
    y = {"PdasLm": eta + rng.standard_normal(n), "PdasLogistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))) * 1.0,
         "PdasPoisson": rng.poisson(np.exp(eta)) * 1.0}[name]
    est = getattr(linear, name)(sequence=list(range(1, 7)))
    Xd = _dev(X)
    est.fit(Xd, y)
    dev, host = est.diagnostics(Xd, _dev(y)), est.diagnostics(X, y)
    assert all(isinstance(dev[kd], torch.Tensor) and dev[kd].device == Xd.device for kd in KINDS)
    link = est._LINK[est.model_type_int]
    cols = np.nonzero(est.beta)[0]
    assert np.array_equal(dev["cols"], cols) and np.array_equal(host["cols"], cols)
    assert dev["positive_definite"] and host["positive_definite"]
    c0 = float(np.ravel(est.coef0)[0])
    iref = inforef.information_reference(X, cols, est.beta[cols], c0, y, None, link, max(n, inforef.device_depth(gpu, n, cols.size)))
    _, _, rel, cond = inforef.se_reference(iref)
    info = linear.bess_base._information_host(link, X[:, cols], est.beta[cols], c0, y, np.ones(n))
    R, pd = gpu.info_factor(info["info"])
    L = iref["loss"]
    phi_rel = LD(2) * L["bound"][0] / L["loss"][0] + LD(8) * inforef.U if link == "identity" else 0
    ref = diagref.diagnostics_reference(X, cols, est.beta[cols], c0, y, None, link, R, host["dispersion"],
                                        diagref.sum_depth(cols.size + 1, host=True), factor_rel=LD(4) * rel, phi_rel=phi_rel)
    d = _np({kd: dev[kd] for kd in KINDS})
    h = {kd: host[kd] for kd in KINDS}
    diagref.check_diagnostics(d, ref, name + " device")
    diagref.check_diagnostics(h, ref, name + " host")
    for kd in KINDS:
        assert (np.abs(d[kd] - h[kd]).astype(LD) <= 2 * ref["bound"][kd]).all(), kd
    sub = est.diagnostics(Xd, y, kinds=["cooks"])
    assert list(sub) == ["cooks", "cols", "dispersion", "positive_definite"]
    assert np.array_equal(sub["cooks"].cpu().numpy(), d["cooks"])


def test_a_singular_information_on_a_device_matrix_gives_nan_leverage_kinds(gpu):
    rng = np.random.default_rng(6)
    X = rng.standard_normal((300, 5))
    X[:, 3] = X[:, 1]
    est = linear.PdasLm()
    est.p, est.beta, est.coef0 = 5, np.array([0.0, 0.5, 0.0, 0.5, -1.0]), 0.1
    y = X @ est.beta + rng.standard_normal(300)
    got = est.diagnostics(_dev(X), y)
    assert got["positive_definite"] is False
    for k in linear.capi.DIAG_LEVERAGE_KINDS:
        assert isinstance(got[k], torch.Tensor) and bool(torch.isnan(got[k]).all()) and got[k].shape == (300,)
    for k in ("response", "pearson", "deviance"):
        assert bool(torch.isfinite(got[k]).all())


def test_device_memory_is_given_back_and_requests_repeat(gpu):
    n, m = 4097, 31
    pr = _sub("f64", n, m)
    t = _dev(pr["vals"])
    y, w = pr["ys"]["logistic"], _dev(pr["w"])
    R, phi = _factor("f64", m), 1.0

    def call(**kw):
        gpu.diagnostics_device(t, pr["cols"], pr["beta"], pr["c"], y, factor=R, dispersion=phi, link="logistic", weight=w,
                               **kw)
        return gpu.process_counters()

    before = gpu.process_counters()
    first = call()
    second = call()
    third = call(kinds=["response"])
    fourth = call(kinds=["cooks"], out=torch.empty((1, n), dtype=torch.float64, device=t.device))
    for c in (first, second, third, fourth):
        assert c["live_device_bytes"] == before["live_device_bytes"]
        assert c["live_pinned_bytes"] == before["live_pinned_bytes"]
    added = second["allocation_requests"] - first["allocation_requests"]
    assert added > 0 and first["allocation_requests"] - before["allocation_requests"] == added
