"""Robust and cluster-robust covariances without a GPU: bess_base.inference(..., cov_type=..., cluster=...) and
inference_survival on a NumPy X (bess_base._sandwich_host / _cox_sandwich_host, fp64 NumPy) against the longdouble
reference and the derived bounds of tests/sandwichref.py; capi.sandwich_table / cox_sandwich_table (scale factors, NaN
rules, the covariance against a longdouble sandwich); every ValueError; the workspace figures and the argument checks of
bessx_meat_device / bessx_sandwich_device, which are made before any device call."""
import ctypes

import numpy as np
import pytest

import coxdiagref
import inforef
import sandwichref
from bess_amd import capi, linear

LD = np.longdouble
LINKS = ["identity", "logistic", "poisson"]
KINDS = ["HC0", "HC1", "HC2", "HC3"]
N, P, MS = 300, 40, 6


def _est(link, beta, coef0):
    est = {"identity": linear.PdasLm, "logistic": linear.PdasLogistic, "poisson": linear.PdasPoisson}[link]()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, coef0
    return est


def _cox(beta):
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = beta.shape[0], beta, 0.0
    return est


_CASES = {}


def _case(link):
    """A model on N rows with a support of 6 of P columns, responses, weights in eighths with zeros, and cluster labels
    (sizes 1 .. 40, shuffled rows, negative and huge values) -- computed once and shared."""
    if link not in _CASES:
        rng = np.random.default_rng(23 + LINKS.index(link))
        X = rng.standard_normal((N, P))
        cols = np.sort(rng.choice(P, MS, replace=False))
        beta = np.zeros(P)
        beta[cols] = rng.standard_normal(MS) * 0.5
        coef0 = 0.3
        eta = X @ beta + coef0
        y = {"identity": eta + rng.standard_normal(N),
             "logistic": (rng.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(float),
             "poisson": rng.poisson(np.exp(eta)).astype(float)}[link]
        w = rng.integers(0, 17, N) / 8.0
        sizes = []
        while sum(sizes) < N:
            sizes.append(min(int(rng.integers(1, 41)), N - sum(sizes)))
        names = rng.choice(np.array([-2 ** 62, -7, 0, 3, 2 ** 40, 2 ** 62] + list(range(100, 100 + len(sizes)))),
                           len(sizes), replace=False)
        labels = rng.permutation(np.repeat(names, sizes)).astype(np.int64)
        _CASES[link] = dict(X=X, cols=cols, beta=beta, coef0=coef0, y=y, w=w, labels=labels)
    return _CASES[link]


def _host_info(cs, link, w):
    return linear.bess_base._information_host(link, cs["X"][:, cs["cols"]], cs["beta"][cs["cols"]], cs["coef0"], cs["y"],
                                              np.ones(N) if w is None else w)


def test_symbols_are_exported():
    for name in ("bessx_meat_device", "bessx_sandwich_device", "bessx_sandwich_workspace", "bessx_op_sandwich_bench"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    for name in ("MeatInput", "SandwichInput", "COV_TYPES", "meat_device", "sandwich_device", "sandwich_workspace",
                 "sandwich_table", "cox_sandwich_table", "op_sandwich_bench"):
        assert hasattr(capi, name)
    assert capi.COV_TYPES == tuple(KINDS)
    assert hasattr(linear.bess_base, "_sandwich_host") and hasattr(linear.bess_base, "_cox_sandwich_host")


@pytest.mark.parametrize("kind,clustered", [(k, False) for k in KINDS] + [("HC0", True), ("HC1", True)])
@pytest.mark.parametrize("link", LINKS)
def test_numpy_route_is_within_the_bounds_of_the_reference(link, kind, clustered):
    cs = _case(link)
    labels = cs["labels"] if clustered else None
    info = _host_info(cs, link, cs["w"])
    R, pd = capi.info_factor(info["info"])
    assert pd
    ref = sandwichref.meat_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"], cs["w"], link, kind,
                                     R, labels, sandwichref.host_depths(N, labels), host=True)
    tb = _est(link, cs["beta"], cs["coef0"]).inference(cs["X"], cs["y"], weight=cs["w"], cov_type=kind, cluster=labels)
    what = "%s %s clustered=%s" % (link, kind, clustered)
    sandwichref.check_meat({"meat": tb["meat"]}, ref, what)
    G = ref["G"]
    assert tb["n_clusters"] == G and tb["cov_type"] == kind and tb["dispersion"] == 1.0 and tb["dof"] == N - MS - 1
    M = MS + 1
    c = {"HC0": 1.0, "HC2": 1.0, "HC3": 1.0,
         "HC1": (G / (G - 1)) * ((N - 1) / (N - M)) if clustered else N / (N - M)}[kind]
    assert tb["scale"] == c
    if kind in ("HC2", "HC3"):
        h = ref["rows"]["h"]
        print("%s: largest leverage %.4f" % (what, float(h.max())))
        assert h.max() <= 0.99
    # the table is sandwich_table's of the same info and meat, and its covariance is the sandwich of these
    again = capi.sandwich_table(info["info"], tb["meat"], info["score"], tb["coef"], kind, N, G)
    for k in ("cov", "se", "z", "p_value"):
        assert np.array_equal(again[k], tb[k]), k
    assert np.array_equal(tb["cov"], tb["cov"].T)
    assert np.array_equal(tb["se"], np.sqrt(np.diag(tb["cov"]))) and np.array_equal(tb["cols"], cs["cols"])


def test_every_row_its_own_cluster_is_hc0():
    cs = _case("logistic")
    est = _est("logistic", cs["beta"], cs["coef0"])
    a = est.inference(cs["X"], cs["y"], weight=cs["w"], cov_type="HC0")
    b = est.inference(cs["X"], cs["y"], weight=cs["w"], cov_type="HC0", cluster=np.arange(N)[::-1].copy())
    args = (cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"], cs["w"], "logistic", "HC0", None)
    ra = sandwichref.meat_reference(*args, None, sandwichref.host_depths(N), host=True)
    rb = sandwichref.meat_reference(*args, np.arange(N), sandwichref.host_depths(N, np.arange(N)), host=True)
    assert (np.abs(a["meat"].astype(LD) - b["meat"].astype(LD)) <= ra["meat_bound"] + rb["meat_bound"]).all()
    assert b["n_clusters"] == N and a["n_clusters"] is None


def test_sandwich_table_against_a_longdouble_sandwich():
    """A well-conditioned problem: info and B formed in longdouble, rounded to fp64 for sandwich_table; the covariance
    against the longdouble sandwich within the bound from the conditioning (sandwichref step 7)."""
    cs = _case("poisson")
    for kind, labels in (("HC0", None), ("HC1", None), ("HC1", cs["labels"]), ("HC3", None)):
        iref = inforef.information_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"], cs["w"],
                                             "poisson", depth=N)
        R, _ = capi.info_factor(iref["info"].astype(np.float64))
        mref = sandwichref.meat_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["coef0"], cs["y"], cs["w"],
                                          "poisson", kind, R, labels, sandwichref.host_depths(N, labels), host=True)
        coef = np.concatenate([[cs["coef0"]], cs["beta"][cs["cols"]]])
        tb = capi.sandwich_table(iref["info"].astype(np.float64), mref["meat"].astype(np.float64),
                                 iref["score"].astype(np.float64), coef, kind, N, mref["G"])
        cov, se, bdiag, bse, cond = sandwichref.covariance_reference(iref["info"], mref["meat"], tb["scale"])
        err = np.abs(tb["se"].astype(LD) - se)
        print("%s clustered=%s: cond(S*) %.3e, se err %.3e against bound %.3e (relative bound %.3e)" % (
            kind, labels is not None, cond, float(err.max()), float(bse.max()), float((bse / se).max())))
        assert tb["positive_definite"] and (bse / se).max() < 1e-6
        assert (err <= bse).all()
        assert (np.abs(np.diag(tb["cov"]).astype(LD) - np.diag(cov)) <= bdiag).all()


def test_scale_factors_and_nan_rules_of_the_tables():
    M = 3
    info, meat = np.diag([4.0, 2.0, 1.0]), np.array([[2.0, 0.5, 0.0], [0.5, 1.0, 0.1], [0.0, 0.1, 3.0]])
    score, coef = np.zeros(M), np.array([1.0, -2.0, 0.5])
    for kind, n, G, c in (("HC0", 10, None, 1.0), ("HC2", 10, None, 1.0), ("HC3", 10, None, 1.0),
                          ("HC1", 10, None, 10 / 7), ("HC0", 10, 4, 1.0), ("HC1", 10, 4, (4 / 3) * (9 / 7))):
        tb = capi.sandwich_table(info, meat, score, coef, kind, n, G)
        assert tb["scale"] == c and tb["n_clusters"] == G and tb["cov_type"] == kind
        cov, se, bdiag, bse, _ = sandwichref.covariance_reference(info, meat, c)
        assert (np.abs(np.diag(tb["cov"]).astype(LD) - np.diag(cov)) <= bdiag).all()
        assert (np.abs(tb["se"].astype(LD) - se) <= bse).all() and tb["positive_definite"] and tb["dispersion"] == 1.0
        assert np.array_equal(tb["z"], coef / tb["se"]) and tb["dof"] == n - M and np.array_equal(tb["meat"], meat)
        assert set(capi.wald_table(info, score, coef, "logistic", 1.0, 10.0)) | {"cov_type", "n_clusters", "scale",
                                                                               "meat"} == set(tb)
    # a non-positive denominator: a NaN table, nothing raised (n <= M without clusters, G = 1 or n <= M with them)
    for kind, n, G in (("HC1", 3, None), ("HC1", 2, None), ("HC1", 10, 1), ("HC1", 3, 2)):
        tb = capi.sandwich_table(info, meat, score, coef, kind, n, G)
        assert np.isnan(tb["scale"])
        for k in ("se", "z", "p_value", "cov"):
            assert np.isnan(tb[k]).all(), (kind, n, G, k)
    # ... while HC0 needs no denominator
    assert np.isfinite(capi.sandwich_table(info, meat, score, coef, "HC0", 2, 1)["se"]).all()
    # an indefinite information matrix: wald_table's rules
    bad = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    for tb in (capi.sandwich_table(bad, meat, score, coef, "HC0", 10), capi.cox_sandwich_table(bad, meat, score, coef, "HC0")):
        assert tb["positive_definite"] is False
        for k in ("se", "z", "p_value", "cov"):
            assert np.isnan(tb[k]).all(), k
    # Cox
    assert capi.cox_sandwich_table(info, meat, score, coef, "HC0")["scale"] == 1.0
    assert capi.cox_sandwich_table(info, meat, score, coef, "HC0", 5)["scale"] == 1.0
    tb = capi.cox_sandwich_table(info, meat, score, coef, "HC1", 5)
    cov, se, bdiag, bse, _ = sandwichref.covariance_reference(info, meat, 5 / 4)
    assert tb["scale"] == 5 / 4 and (np.abs(np.diag(tb["cov"]).astype(LD) - np.diag(cov)) <= bdiag).all()
    assert (np.abs(tb["se"].astype(LD) - se) <= bse).all()
    assert np.isnan(capi.cox_sandwich_table(info, meat, score, coef, "HC1", 1)["se"]).all()
    empty = capi.cox_sandwich_table(np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0), np.zeros(0), "HC0")
    assert empty["se"].shape == (0,) and empty["positive_definite"] is True
    for kind, G in (("HC1", None), ("HC2", None), ("HC3", 4)):
        with pytest.raises(ValueError):
            capi.cox_sandwich_table(info, meat, score, coef, kind, G)
    for kind in ("HC2", "HC3"):
        with pytest.raises(ValueError):
            capi.sandwich_table(info, meat, score, coef, kind, 10, 4)
    with pytest.raises(ValueError):
        capi.sandwich_table(info, meat, score, coef, "HC4", 10)
    with pytest.raises(ValueError):
        capi.sandwich_table(info, meat[:2, :2], score, coef, "HC0", 10)


def test_every_value_error():
    cs = _case("logistic")
    est = _est("logistic", cs["beta"], cs["coef0"])
    X, y, lab = cs["X"], cs["y"], cs["labels"]
    with pytest.raises(ValueError, match="cluster.size"):
        est.inference(X, y, cov_type="HC0", cluster=lab[:-1])
    with pytest.raises(ValueError, match="integer"):
        est.inference(X, y, cov_type="HC0", cluster=lab.astype(np.float64))
    with pytest.raises(ValueError, match="cov_type"):
        est.inference(X, y, cov_type="HC4")
    with pytest.raises(ValueError, match="cov_type"):
        est.inference(X, y, cov_type="robust", cluster=lab)
    with pytest.raises(ValueError, match="model"):
        est.inference(X, y, cluster=lab)
    for kind in ("HC2", "HC3"):
        with pytest.raises(ValueError, match="not available"):
            est.inference(X, y, cov_type=kind, cluster=lab)
    multi = linear.PdasLm()
    multi.p, multi.beta, multi.coef0 = P, np.zeros((P, 2)), np.zeros(2)
    with pytest.raises(ValueError, match="2-D beta"):
        multi.inference(X, y, cov_type="HC0")
    # Cox
    rng = np.random.default_rng(3)
    ys = np.column_stack([rng.integers(0, 50, N) / 4.0, (rng.uniform(size=N) < 0.7) * 1.0])
    cox = _cox(cs["beta"])
    for kind, cl in (("HC1", None), ("HC2", None), ("HC3", None), ("HC2", lab), ("model", lab), ("HC9", None)):
        with pytest.raises(ValueError):
            cox.inference_survival(X, ys, cov_type=kind, cluster=cl)
    with pytest.raises(ValueError, match="cluster.size"):
        cox.inference_survival(X, ys, cov_type="HC0", cluster=lab[:5])
    with pytest.raises(ValueError, match="integer"):
        cox.inference_survival(X, ys, cov_type="HC0", cluster=lab * 0.5)
    # a fitted Cox model keeps inference() None, also with a robust cov_type
    assert cox.inference(X, y, cov_type="HC0") is None


def test_defaults_return_exactly_what_the_parent_returned():
    for link in LINKS:
        cs = _case(link)
        for w in (None, cs["w"]):
            tb = _est(link, cs["beta"], cs["coef0"]).inference(cs["X"], cs["y"], weight=w)
            info = _host_info(cs, link, w)
            want = capi.wald_table(info["info"], info["score"], np.concatenate([[cs["coef0"]], cs["beta"][cs["cols"]]]),
                                   link, info["loss"], info["sum_w"])
            want["cols"] = cs["cols"]
            assert list(tb) == list(want)
            for k in want:
                assert np.array_equal(np.asarray(tb[k]), np.asarray(want[k]), equal_nan=True), (link, k)
    cs = _case("logistic")
    rng = np.random.default_rng(4)
    ys = np.column_stack([rng.integers(0, 50, N) / 4.0, (rng.uniform(size=N) < 0.7) * 1.0])
    for ties in ("order", "breslow"):
        tb = _cox(cs["beta"]).inference_survival(cs["X"], ys, weight=cs["w"], ties=ties)
        got = linear.bess_base._cox_information_host(cs["X"][:, cs["cols"]], cs["beta"][cs["cols"]], ys[:, 0], ys[:, 1],
                                                     cs["w"], ties)
        want = capi.cox_wald_table(got["info"], got["score"], cs["beta"][cs["cols"]], got["n_events"])
        want.update(cols=cs["cols"], loglik=float(got["loglik"]), residual_sum=float(got["residual_sum"]))
        assert list(tb) == list(want)
        for k in want:
            assert np.array_equal(np.asarray(tb[k]), np.asarray(want[k]), equal_nan=True), (ties, k)


@pytest.mark.parametrize("clustered", [False, True])
@pytest.mark.parametrize("ties", ["order", "breslow"])
def test_cox_numpy_route_is_within_the_bounds_of_the_reference(ties, clustered):
    rng = np.random.default_rng(51)
    m = 6
    X = rng.standard_normal((N, P))
    cols = np.sort(rng.choice(P, m, replace=False))
    beta = np.zeros(P)
    beta[cols] = rng.standard_normal(m) / np.sqrt(m)
    time = rng.integers(0, int(2.5 * N), N) / 8.0
    status = (rng.uniform(size=N) < 0.7).astype(np.float64)
    w = rng.integers(0, 17, N) / 8.0
    labels = _case("logistic")["labels"] if clustered else None
    dref = coxdiagref.cox_diag_reference(X, cols, beta[cols], time, status, w, ties, None, None, coxdiagref.host_depths(m))
    sd, gd = sandwichref.host_depths(N, labels)
    ref = sandwichref.rows_reference(dref["score"], dref["score_bound"], labels, sd, gd)
    kind = "HC1" if clustered else "HC0"
    tb = _cox(beta).inference_survival(X, np.column_stack([time, status]), weight=w, ties=ties, cov_type=kind,
                                       cluster=labels)
    sandwichref.check_meat({"meat": tb["meat"]}, ref, "cox %s clustered=%s" % (ties, clustered))
    G = ref["G"] if clustered else None
    assert tb["n_clusters"] == G and tb["scale"] == (G / (G - 1) if clustered else 1.0) and tb["cov_type"] == kind
    plain = _cox(beta).inference_survival(X, np.column_stack([time, status]), weight=w, ties=ties)
    assert tb["dof"] == plain["dof"] and tb["loglik"] == plain["loglik"] and np.array_equal(tb["score"], plain["score"])
    host = linear.bess_base._cox_information_host(X[:, cols], beta[cols], time, status, w, ties)
    again = capi.cox_sandwich_table(host["info"], tb["meat"], host["score"], beta[cols], kind, G)
    for k in ("cov", "se", "z", "p_value"):
        assert np.array_equal(again[k], tb[k]), k
    # an empty model: empty tables
    e = _cox(np.zeros(P)).inference_survival(X, np.column_stack([time, status]), cov_type="HC0", cluster=labels)
    assert e["se"].shape == (0,) and e["meat"].shape == (0, 0) and e["positive_definite"] is True


def test_workspace_needs_no_device_and_states_the_depths():
    n, m = 100000, 200
    plain = capi.sandwich_workspace(n, m, link="logistic", weighted=True)
    nd, rps, slabs = capi.info_workspace(n, m, link="logistic", weighted=True)
    nv = (n + 1) // 2 * 2
    assert plain["doubles"] == nd + 3 + 2 * nv + m + 1 and (plain["rows_per_slab"], plain["slabs"]) == (rps, slabs)
    assert plain["cluster_slabs"] == 0 and plain["sum_depth"] == 0 and plain["sq_depth"] == 0
    hc3 = capi.sandwich_workspace(n, m, link="logistic", weighted=True, kind="HC3")
    assert hc3["doubles"] > plain["doubles"] + nv
    run = capi.SANDWICH_RUN
    for r, want in ((1, 1), (8, 8), (run, run), (run + 1, run + 1), (2 * run, run + 1), (n, run + (n + run - 1) // run - 1)):
        ws = capi.sandwich_workspace(n, m, n_clusters=max(n // r, 1), max_cluster_rows=r)
        assert ws["sum_depth"] == want, (r, ws)
        G = max(n // r, 1)
        assert ws["sq_depth"] == (G + 255) // 256 + 8
        _, crps, cslabs = capi.info_workspace(G, m)
        assert (ws["cluster_rows_per_slab"], ws["cluster_slabs"]) == (crps, cslabs)
        assert ws["doubles"] >= plain["doubles"] + G * (m + 1)
    # nothing n x M is stored: with clusters of 8 rows the scratch stays far below n * M doubles
    assert capi.sandwich_workspace(n, m, n_clusters=n // 8, max_cluster_rows=8)["doubles"] < n * (m + 1) // 2
    for bad in (dict(n=0, m=1), dict(n=10, m=-1), dict(n=10, m=1, n_clusters=11, max_cluster_rows=1),
                dict(n=10, m=1, n_clusters=2, max_cluster_rows=0)):
        with pytest.raises(capi.BessxError) as e:
            capi.sandwich_workspace(**bad)
        assert e.value.code == 1
    with pytest.raises(capi.BessxError) as e:
        capi.sandwich_workspace(10, 1024)
    assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
    with pytest.raises(ValueError):
        capi.sandwich_workspace(10, 1, kind="HC4")


def test_argument_checks_come_before_any_device_call():
    """Pointers that are never dereferenced: every one of these is refused on the arguments alone."""
    L = capi.lib()
    cols = np.array([0, 2], dtype=np.int32)
    beta, y, lab = np.array([0.5, -0.5]), np.zeros(4), np.zeros(4, dtype=np.int64)
    out = np.zeros(16)

    def sandwich(**kw):
        a = capi.SandwichInput()
        a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1024, 0, 3, 1, 4, 3
        a.cols, a.m, a.beta, a.coef0, a.link = capi._ip(cols), 2, capi._dp(beta), 0.0, 1
        a.y_host, a.info, a.info_ld, a.score, a.meat, a.meat_ld = capi._dp(y), out.ctypes.data, 3, out.ctypes.data, \
            out.ctypes.data, 3
        for k, v in kw.items():
            setattr(a, k, v)
        loss, sw, G = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        rc = L.bessx_sandwich_device(ctypes.byref(a), ctypes.byref(loss), ctypes.byref(sw), ctypes.byref(G))
        return rc, capi.last_error()

    labp = lab.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    for kw, text in ((dict(kind=4), "kind must be one of"), (dict(kind=-1), "kind must be one of"),
                     (dict(kind=2), "need the factor"), (dict(kind=3, factor=capi._dp(out), factor_ld=2), "factor_ld"),
                     (dict(kind=2, factor=capi._dp(np.full(9, np.nan)), factor_ld=3), "must be finite"),
                     (dict(kind=2, factor=capi._dp(out), factor_ld=3, cluster_host=labp), "BESSX_HC0 or BESSX_HC1 only"),
                     (dict(cluster_host=labp, cluster_dev=1024), "not both"),
                     (dict(cluster_dev=1024, cluster_dtype=2), "BESSX_I64 or BESSX_I32"),
                     (dict(cluster_dev=1024, cluster_stride=-1), "strides must be non-negative"),
                     (dict(meat=None), "null argument"), (dict(meat_ld=2), "meat_ld"), (dict(info_ld=2), "info_ld"),
                     (dict(x_row_stride=-1), "strides must be non-negative"), (dict(link=7), "unknown link"),
                     (dict(coef0=float("inf")), "coef0 must be finite")):
        rc, msg = sandwich(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)

    def meat(**kw):
        a = capi.MeatInput()
        a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = 1024, 0, 3, 1, 4, 3
        a.cols, a.m, a.intercept, a.meat, a.meat_ld, a.sums = capi._ip(cols), 2, 1, out.ctypes.data, 3, out.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        G = ctypes.c_int(0)
        rc = L.bessx_meat_device(ctypes.byref(a), ctypes.byref(G))
        return rc, capi.last_error()

    for kw, text in ((dict(m=0, intercept=0), "needs the intercept"), (dict(meat_ld=2), "meat_ld"),
                     (dict(u_host=capi._dp(y), u_dev=1024), "not both"), (dict(sums=None), "null argument"),
                     (dict(x_dtype=5), "dtype must be"), (dict(cluster_host=labp, cluster_dev=1024), "not both"),
                     (dict(m=4), "m must lie in")):
        rc, msg = meat(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    big = np.arange(1025, dtype=np.int32)
    rc, msg = meat(cols=capi._ip(big), m=1025, p=2000, intercept=0, meat_ld=2000)
    assert rc == 3 and "at most 1024" in msg
    rc, msg = meat(cols=capi._ip(big), m=1024, p=2000, intercept=1, meat_ld=2000)
    assert rc == 3 and "at most 1024" in msg
