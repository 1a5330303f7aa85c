"""The meat of the robust and cluster-robust covariances on an X already in GPU memory (bessx_meat_device,
bessx_sandwich_device, bess_amd/csrc/bessx_k_sandwich.hip) against NumPy in np.longdouble on the host copy of the same
values, within the bounds derived in tests/sandwichref.py (the addition depths are those the library reports through
capi.sandwich_workspace).  Shapes, layouts (every element outside the view a NaN) and the forms of y and weight are those
of tests/test_info_gpu.py.  Cluster labels: one cluster of all rows (longer than a run of 64 for n > 64), every row its
own cluster, random sizes 1 .. 40 with shuffled rows and negative / huge / non-contiguous labels, the same clusters with
sorted labels (the 16-byte loads of a column-contiguous source), a cluster of 100 rows among short ones, and sorted
clusters with one of several runs across the workgroup edge of the cluster-sum kernel (positions 255 / 256 of the run
table) and rows of S on both sides of the first slab edge of the sweep over S."""
import numpy as np
import pytest

import coxdiagref
import inforef
import sandwichref
from bess_amd import capi, linear

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
DT = {"f64": np.float64, "f32": np.float32}
LAYOUTS = ["C", "F", "T", "two_strides", "odd_offset"]
LINKS = ["identity", "logistic", "poisson"]
P = 600
NS, MS = (1, 127, 4097), (0, 1, 14, 15, 16, 31, 200)
LABELS = ["one", "own", "random", "sorted", "long", "edge"]
# (kind, labels) per call, rotated over the supports, links and row counts
CONFIGS = [("HC0", None), ("HC1", "random"), ("HC3", None), ("HC0", "sorted"), ("HC2", None), ("HC1", "special")]
SPECIAL = ["one", "own", "long", "edge"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _embed(layout, vals):
    """(base host array that holds vals in the layout under test, NaN everywhere else; base tensor -> the n x p view)"""
    n, p = vals.shape
    if layout == "C":  # row-major
        return vals.copy(), (lambda t: t)
    if layout == "F":  # column-major with a padded leading dimension: aligned columns (the 16-byte loads), NaN rows >= n
        b = np.full((p, (n + 3) // 4 * 4), np.nan, dtype=vals.dtype)
        b[:, :n] = vals.T
        return b, (lambda t: t[:, :n].T)
    if layout == "T":  # a transposed view that starts on an odd element: column-contiguous, element loads
        b = np.full((p, n + 3), np.nan, dtype=vals.dtype)
        b[:, 1:1 + n] = vals.T
        return b, (lambda t: t[:, 1:1 + n].T)
    if layout == "two_strides":
        b = np.full((2 * n, 3 * p), np.nan, dtype=vals.dtype)
        b[::2, ::3] = vals
        return b, (lambda t: t[::2, ::3])
    if layout == "odd_offset":  # row-contiguous, first element at an odd offset
        b = np.full((n, p + 5), np.nan, dtype=vals.dtype)
        b[:, 3:3 + p] = vals
        return b, (lambda t: t[:, 3:3 + p])
    raise AssertionError(layout)


_VALS, _PROBLEMS, _REFS, _LABELS, _FACTORS = {}, {}, {}, {}, {}


def _vals(dt, n, p=P):
    if (dt, n, p) not in _VALS:
        _VALS[(dt, n, p)] = np.random.default_rng(n + (1 if dt == "f32" else 0)).standard_normal((n, p)).astype(DT[dt])
    return _VALS[(dt, n, p)]


def _problem(dt, n, m, p=P):
    """One model per (dtype, n, m), the same logical values under every layout (the construction of
    tests/test_info_gpu.py)."""
    key = (dt, n, m, p)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(1000 * n + 10 * m + (7 if dt == "f32" else 0))
        vals = _vals(dt, n, p)
        cols = np.sort(rng.choice(p, m, replace=False)).astype(np.int32)
        beta = rng.standard_normal(m) / np.sqrt(max(m, 1))
        c = 0.3
        eta = vals[:, cols].astype(np.float64) @ beta + c
        ys = {"identity": eta + rng.standard_normal(n),
              "logistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(float),
              "poisson": rng.poisson(np.exp(np.clip(eta, -5, 3))).astype(float)}
        w = rng.integers(0, 17, n) / 8.0
        _PROBLEMS[key] = dict(vals=vals, cols=cols, beta=beta, c=c, ys=ys, w=w)
    return _PROBLEMS[key]


def _labels(gpu, name, n, m=31):
    """n int64 labels of the named kind (shared, never changed)."""
    key = (name, n)
    if key not in _LABELS:
        rng = np.random.default_rng(77 + n)
        if name == "one":
            lab = np.full(n, -5, dtype=np.int64)
        elif name == "own":
            lab = (rng.permutation(n).astype(np.int64) - n // 2) * 1000003
        elif name in ("random", "sorted"):
            sizes = []
            while sum(sizes) < n:
                sizes.append(min(int(rng.integers(1, 41)), n - sum(sizes)))
            names = np.sort(rng.choice(np.arange(-4 * len(sizes), 4 * len(sizes)), len(sizes), replace=False)) * (2 ** 40 + 1)
            names[0], names[-1] = -2 ** 62, 2 ** 62
            lab = np.repeat(names.astype(np.int64), sizes)
            if name == "random":
                lab = np.random.default_rng(78 + n).permutation(lab)
        elif name == "long":  # one cluster of min(n, 100) rows (longer than a run of 64) among clusters of one row
            lab = np.arange(n, dtype=np.int64) + 10
            lab[rng.permutation(n)[:min(n, 100)]] = 3
        elif name == "edge":  # sorted labels: single rows, then ONE cluster of several runs whose runs lie across
            # position 255 / 256 of the run table (the workgroup edge of the cluster-sum kernel), then clusters of 8; the
            # rows 63 / 64 of S (the first slab edge of the sweep over S) lie among the single rows
            singles = min(254, n // 3)
            long_rows = min(200, n - singles)
            sizes = [1] * singles + [long_rows] + [8] * ((n - singles - long_rows) // 8)
            sizes += [n - sum(sizes)] if n > sum(sizes) else []
            lab = np.repeat(np.arange(len(sizes), dtype=np.int64) * 5 - 1000, sizes)
            if n >= 454:
                assert singles == 254 and long_rows > 3 * 64  # (runs 254 .. 257 belong to the long cluster)
        else:
            raise AssertionError(name)
        _LABELS[key] = lab
    return _LABELS[key]


def _forms(pr, link, fi, wi):
    """y and weight as passed: host array, float64 device array, strided device view, float32 device array; wi = 0 is
    no weight.  Returns (y, weight, y is float32)."""
    y, w = pr["ys"][link], pr["w"]
    ys = [y, _dev(y), _dev(np.column_stack([y, y]))[:, 1], _dev(y.astype(np.float32))]
    ws = [None, w, _dev(w), _dev(np.column_stack([w, w, w]))[:, 2], _dev(w.astype(np.float32))]
    return ys[fi], ws[wi], fi == 3


def _factor(pr, link, y, w):
    """(R, positive definite) from the NumPy route's information: R is fp64 DATA, the same under every layout."""
    n = pr["vals"].shape[0]
    key = (id(pr), link, y.dtype.str, w is None)
    if key not in _FACTORS:
        info = linear.bess_base._information_host(link, pr["vals"][:, pr["cols"]].astype(np.float64), pr["beta"], pr["c"],
                                                  y.astype(np.float64), np.ones(n) if w is None else w)["info"]
        _FACTORS[key] = capi.info_factor(info)
    return _FACTORS[key]


def _config(gpu, n, m, ni, mi, li):
    """(kind, label name or None) of the call: HC2 / HC3 fall back to HC1 where the information cannot be inverted
    (fewer than 4 rows per coefficient)."""
    kind, lab = CONFIGS[(mi + li + ni) % len(CONFIGS)]
    if lab == "special":
        lab = SPECIAL[(mi + ni) % len(SPECIAL)]
    if kind in ("HC2", "HC3") and n < 4 * (m + 1):
        kind = "HC1"
    return kind, lab


def _ref(gpu, dt, n, m, link, y32, weighted, kind, lab, p=P):
    key = (dt, n, m, link, y32, weighted, kind, lab, p)
    if key not in _REFS:
        pr = _problem(dt, n, m, p)
        y = pr["ys"][link].astype(np.float32) if y32 else pr["ys"][link]
        w = pr["w"] if weighted else None
        labels = None if lab is None else _labels(gpu, lab, n, m)
        R = _factor(pr, link, y, w)[0] if kind in ("HC2", "HC3") else None
        _REFS[key] = sandwichref.meat_reference(pr["vals"], pr["cols"], pr["beta"], pr["c"], y, w, link, kind, R, labels,
                                                sandwichref.device_depths(gpu, n, m, labels))
    return _REFS[key]


def _call(gpu, t, pr, link, y, w, kind, labels, R=None):
    return gpu.sandwich_device(t, pr["cols"], pr["beta"], pr["c"], y, link=link, weight=w, kind=kind,
                               factor=R if kind in ("HC2", "HC3") else None, cluster=labels)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_meat_is_within_the_bounds_and_the_information_keeps_its_bits(gpu, dt, layout, n):
    base, view = _embed(layout, _vals(dt, n))
    t = view(_dev(base))
    assert tuple(t.shape) == (n, P)
    ni = NS.index(n)
    for mi, m in enumerate(MS):
        pr = _problem(dt, n, m)
        for li, link in enumerate(LINKS):
            fi, wi = (mi + li) % 4, (mi + 2 * li + ni) % 5
            y, w, y32 = _forms(pr, link, fi, wi)
            kind, lab = _config(gpu, n, m, ni, mi, li)
            yh = pr["ys"][link].astype(np.float32) if y32 else pr["ys"][link]
            R = None
            if kind in ("HC2", "HC3"):
                R, pd = _factor(pr, link, yh, pr["w"] if wi > 0 else None)
                if not pd:
                    kind = "HC1"
            labels = None if lab is None else _labels(gpu, lab, n, m)
            if lab is not None and (mi + li) % 2:  # (labels in device memory every other time)
                labels_arg = _dev(labels)
            else:
                labels_arg = labels
            ref = _ref(gpu, dt, n, m, link, y32, wi > 0, kind, lab)
            what = "%s %s n=%d m=%d %s y%d w%d %s %s" % (dt, layout, n, m, link, fi, wi, kind, lab)
            got = _call(gpu, t, pr, link, y, w, kind, labels_arg, R)
            assert got["meat"].shape == (m + 1, m + 1)
            sandwichref.check_meat({"meat": got["meat"]}, ref, what)
            assert got["n_clusters"] == ref["G"], what
            if kind in ("HC2", "HC3"):
                assert ref["rows"]["h"].max() <= 0.99, what
            info = gpu.information_device(t, pr["cols"], pr["beta"], pr["c"], y, link=link, weight=w)
            assert np.array_equal(got["info"], info["info"]) and np.array_equal(got["score"], info["score"]), what
            assert got["loss"] == info["loss"] and got["sum_w"] == info["sum_w"], what


@pytest.mark.parametrize("lab", LABELS)
def test_every_kind_of_labels_and_the_sum_vector(gpu, lab):
    """meat_device with a row scalar u: meat, the sum vector and (through them) S within their bounds; u as a host and as
    a device array, labels as a host and as a device array, give the same bits."""
    for dt, layout, n, m in (("f64", "F", 4097, 31), ("f32", "C", 127, 15), ("f64", "T", 127, 0), ("f64", "odd_offset", 1, 1)):
        pr = _problem(dt, n, m)
        base, view = _embed(layout, pr["vals"])
        t = view(_dev(base))
        u = np.random.default_rng(n + m).standard_normal(n)
        labels = _labels(gpu, lab, n, m)
        sd, gd = sandwichref.device_depths(gpu, n, m, labels)
        Z = np.column_stack([np.ones(n), pr["vals"][:, pr["cols"]].astype(np.float64)])
        ref = sandwichref.clustered_reference(Z, u, None, labels, sd, gd)
        got = gpu.meat_device(t, pr["cols"], u=u, cluster=labels)
        sandwichref.check_meat(got, ref, "%s %s %s n=%d m=%d" % (lab, dt, layout, n, m))
        assert got["n_clusters"] == ref["G"] == np.unique(labels).size
        for dl in (_dev(labels), _dev(np.column_stack([labels, labels]))[:, 1]):  # (contiguous and strided)
            again = gpu.meat_device(t, pr["cols"], u=_dev(u), cluster=dl)
            assert np.array_equal(got["meat"], again["meat"]) and np.array_equal(got["sums"], again["sums"])
        i32 = gpu.meat_device(t, pr["cols"], u=u, cluster=_dev((labels % 100003).astype(np.int32))[:])
        assert i32["n_clusters"] == np.unique(labels % 100003).size
    # without labels: one sweep over x, with and without u
    pr = _problem("f64", 4097, 31)
    t = _dev(pr["vals"])
    Z = np.column_stack([np.ones(4097), pr["vals"][:, pr["cols"]]])
    for uu in (None, u if u.size == 4097 else np.random.default_rng(5).standard_normal(4097)):
        ref = sandwichref.unclustered_reference(Z, uu, None, sandwichref.device_depths(gpu, 4097, 31)[1])
        got = gpu.meat_device(t, pr["cols"], u=uu)
        sandwichref.check_meat(got, ref, "no labels, u %s" % (uu is not None))
        assert got["n_clusters"] is None


def test_a_broadcast_label_vector_of_stride_zero_is_one_cluster(gpu):
    """torch.tensor([g]).cuda().expand(n): a device view of ONE element with stride 0.  One element is read; the results
    are the bits of np.full(n, g)."""
    for n, m in ((4097, 31), (1, 1)):
        pr = _problem("f64", n, m)
        t = _dev(pr["vals"])
        y, w = pr["ys"]["logistic"], pr["w"]
        for tdt, npdt in ((torch.int64, np.int64), (torch.int32, np.int32)):
            one = torch.tensor([-7], dtype=tdt).cuda().expand(n)
            assert one.untyped_storage().nbytes() == np.dtype(npdt).itemsize and (n == 1 or one.stride() == (0,))
            want = _call(gpu, t, pr, "logistic", y, w, "HC1", np.full(n, -7, dtype=np.int64))
            got = _call(gpu, t, pr, "logistic", y, w, "HC1", one)
            assert got["n_clusters"] == want["n_clusters"] == 1 and np.array_equal(got["meat"], want["meat"])
            a = gpu.meat_device(t, pr["cols"], cluster=one)
            b = gpu.meat_device(t, pr["cols"], cluster=np.full(n, -7, dtype=np.int64))
            assert a["n_clusters"] == 1 and np.array_equal(a["meat"], b["meat"]) and np.array_equal(a["sums"], b["sums"])


def test_clustered_meat_is_the_same_bits_under_every_layout_and_twice(gpu):
    """The three access shapes of the cluster-sum kernel do the same arithmetic in the same order, and u comes from a
    predictor pass with threads along rows under every layout."""
    n, m = 4097, 31
    pr = _problem("f64", n, m)
    y, w = pr["ys"]["poisson"], pr["w"]
    for lab in ("random", "sorted", "one"):
        labels = _labels(gpu, lab, n, m)
        first = None
        for layout in LAYOUTS:
            base, view = _embed(layout, pr["vals"])
            t = view(_dev(base))
            a = _call(gpu, t, pr, "poisson", y, w, "HC1", labels)
            b = _call(gpu, t, pr, "poisson", _dev(y), _dev(w), "HC1", _dev(labels))
            assert np.array_equal(a["meat"], b["meat"]) and np.array_equal(a["info"], b["info"]), (lab, layout)
            if first is None:
                first = a
            assert np.array_equal(a["meat"], first["meat"]), (lab, layout)
    # ... and without labels the same call gives the same bits, also on a second stream
    t = _dev(pr["vals"])
    R, pd = _factor(pr, "poisson", y, w)
    assert pd
    a = _call(gpu, t, pr, "poisson", y, w, "HC3", None, R)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = gpu.sandwich_device(t, pr["cols"], pr["beta"], pr["c"], y, link="poisson", weight=w, kind="HC3", factor=R,
                                stream=s.cuda_stream)
    assert np.array_equal(a["meat"], b["meat"])


def test_a_cluster_does_not_depend_on_where_it_lies_or_on_the_layout(gpu):
    """S(g, :) is a function of the cluster's rows in their order and of u.  150 rows as the only cluster of a design
    of their own (row-major, u = ones), and the same rows scattered through 4097 (column-major, shuffled labels) with
    u = 1 on them and 0 elsewhere: every other cluster sums to an exact zero, so the sum vector and the meat -- one
    product per entry and additions of zeros -- must be the same bits."""
    pr = _problem("f64", 4097, 31)
    rows = np.sort(np.random.default_rng(9).choice(4097, 150, replace=False))
    small = np.ascontiguousarray(pr["vals"][rows])
    a = gpu.meat_device(_dev(small), pr["cols"], cluster=np.zeros(150, dtype=np.int64))
    lab = _labels(gpu, "random", 4097).copy()
    lab[rows] = 12345
    u = np.zeros(4097)
    u[rows] = 1.0
    for layout in LAYOUTS:
        base, view = _embed(layout, pr["vals"])
        b = gpu.meat_device(view(_dev(base)), pr["cols"], u=u, cluster=lab)
        assert a["n_clusters"] == 1 and b["n_clusters"] > 100
        assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["meat"], b["meat"]), layout
    ref = sandwichref.clustered_reference(np.column_stack([np.ones(150), small[:, pr["cols"]]]), None, None,
                                          np.zeros(150, dtype=np.int64),
                                          *sandwichref.device_depths(gpu, 150, 31, np.zeros(150, dtype=np.int64)))
    assert (np.abs(a["sums"].astype(LD) - ref["sums"]) <= ref["sums_bound"]).all()
    assert np.array_equal(a["meat"], np.outer(a["sums"], a["sums"]))


@pytest.mark.parametrize("kind", ["HC2", "HC3"])
def test_a_row_of_leverage_near_one(gpu, kind):
    n, p, m = 127, 20, 5
    rng = np.random.default_rng(31)
    vals = rng.standard_normal((n, p))
    cols = np.array([1, 4, 9, 12, 17], dtype=np.int32)
    vals[5, cols[2]] = 40.0  # one far point in one column: its leverage is close to 40^2 / (40^2 + n)
    beta = rng.standard_normal(m) * 0.1
    y = vals[:, cols] @ beta + 0.2 + rng.standard_normal(n)
    pr = dict(vals=vals, cols=cols, beta=beta, c=0.2)
    info = linear.bess_base._information_host("identity", vals[:, cols], beta, 0.2, y, np.ones(n))["info"]
    R, pd = capi.info_factor(info)
    assert pd
    ref = sandwichref.meat_reference(vals, cols, beta, 0.2, y, None, "identity", kind, R, None,
                                     sandwichref.device_depths(gpu, n, m))
    h = ref["rows"]["h"]
    print("%s: largest leverage %.4f, bound on u there %.3e (u %.3e)" % (
        kind, float(h.max()), float(ref["rows"]["bu"][5]), float(ref["rows"]["u"][5])))
    assert 0.9 < h.max() <= 0.99 and int(np.argmax(h)) == 5
    for layout in ("C", "F"):
        base, view = _embed(layout, vals)
        got = _call(gpu, view(_dev(base)), pr, "identity", y, None, kind, None, R)
        sandwichref.check_meat({"meat": got["meat"]}, ref, "%s %s" % (kind, layout))
        lev = gpu.diagnostics_device(view(_dev(base)), cols, beta, 0.2, y, factor=R, kinds=("leverage",))["leverage"]
        assert abs(LD(float(lev[5])) - h[5]) <= ref["rows"]["bh"][5]


def test_every_row_its_own_cluster_agrees_with_hc0(gpu):
    for dt, layout, n, m in (("f64", "F", 4097, 31), ("f32", "C", 127, 14)):
        pr = _problem(dt, n, m)
        base, view = _embed(layout, pr["vals"])
        t = view(_dev(base))
        y, w = pr["ys"]["logistic"], pr["w"]
        own = _labels(gpu, "own", n)
        a = _call(gpu, t, pr, "logistic", y, w, "HC0", None)
        b = _call(gpu, t, pr, "logistic", y, w, "HC0", own)
        ra = _ref(gpu, dt, n, m, "logistic", False, True, "HC0", None)
        rb = _ref(gpu, dt, n, m, "logistic", False, True, "HC0", "own")
        err = np.abs(a["meat"].astype(LD) - b["meat"].astype(LD))
        print("CR0 with every row its own cluster against HC0: %.3e against %.3e" % (
            float(err.max()), float((ra["meat_bound"] + rb["meat_bound"]).max())))
        assert (err <= ra["meat_bound"] + rb["meat_bound"]).all() and b["n_clusters"] == n


@pytest.mark.parametrize("layout", ["C", "F"])
@pytest.mark.parametrize("lab", [None, "random", "sorted"])
def test_a_nan_inside_the_support_propagates_and_one_outside_does_not(gpu, layout, lab):
    """A NaN at x(i, cols[k]) makes eta_i and with it g_i = u_i NaN: without labels every entry of the meat is a sum over
    all rows and is NaN; with labels s_g of row i's cluster is NaN in every entry, and so is the meat.  A NaN in a column
    outside the support or in the padding around the view is never read."""
    n, m, i, k = 127, 31, 77, 9
    pr = _problem("f64", n, m)
    labels = None if lab is None else _labels(gpu, lab, n, m)
    vals = pr["vals"].copy()
    vals[i, pr["cols"][k]] = np.nan
    base, view = _embed(layout, vals)
    got = _call(gpu, view(_dev(base)), pr, "logistic", pr["ys"]["logistic"], pr["w"], "HC0", labels)
    assert np.isnan(got["meat"]).all()
    # the same NaN reaches meat_device through the column alone: row k + 1 and column k + 1, nothing else
    mt = gpu.meat_device(view(_dev(base)), pr["cols"], cluster=labels)
    want = np.zeros((m + 1, m + 1), dtype=bool)
    want[k + 1, :] = want[:, k + 1] = True
    assert np.array_equal(np.isnan(mt["meat"]), want)
    vals = pr["vals"].copy()
    vals[:, np.setdiff1d(np.arange(P), pr["cols"])] = np.nan
    base, view = _embed(layout, vals)
    got = _call(gpu, view(_dev(base)), pr, "logistic", pr["ys"]["logistic"], pr["w"], "HC0", labels)
    sandwichref.check_meat({"meat": got["meat"]}, _ref(gpu, "f64", n, m, "logistic", False, True, "HC0", lab),
                           "NaN outside the support")


@pytest.mark.parametrize("layout", ["C", "F"])
def test_the_largest_support_and_one_past_it(gpu, layout):
    n, p, m = 127, 1100, 1023
    pr = _problem("f64", n, m, p)
    base, view = _embed(layout, pr["vals"])
    t = view(_dev(base))
    y, w = pr["ys"]["logistic"], pr["w"]
    for lab in (None, "random"):
        labels = None if lab is None else _labels(gpu, lab, n, m)
        ref = _ref(gpu, "f64", n, m, "logistic", False, True, "HC0", lab, p)
        got = _call(gpu, t, pr, "logistic", y, w, "HC0", labels)
        sandwichref.check_meat({"meat": got["meat"]}, ref, "m + 1 = 1024 %s %s" % (layout, lab))
    for labels in (None, _labels(gpu, "random", n)):
        with pytest.raises(gpu.BessxError) as e:
            gpu.sandwich_device(t, np.arange(1024), np.zeros(1024), 0.0, y, link="logistic", cluster=labels)
        assert e.value.code == 3 and "m + 1 must be at most 1024" in str(e.value)
        with pytest.raises(gpu.BessxError) as e:
            gpu.meat_device(t, np.arange(1024), cluster=labels)
        assert e.value.code == 3 and "at most 1024" in str(e.value)
    # a dense source without the intercept may have 1024 columns
    got = gpu.meat_device(t, np.arange(1024), cluster=_labels(gpu, "random", n), intercept=False)
    Y = pr["vals"][:, :1024]
    ref = sandwichref.rows_reference(Y, np.zeros_like(Y), _labels(gpu, "random", n),
                                     *sandwichref.device_depths(gpu, n, 1024, _labels(gpu, "random", n), intercept=False))
    sandwichref.check_meat(got, ref, "1024 dense columns " + layout)


_COX = {}


def _cox_case(m):
    if m not in _COX:
        n, p = 300, 40
        rng = np.random.default_rng(61 + m)
        X = rng.standard_normal((n, p))
        cols = np.sort(rng.choice(p, m, replace=False))
        beta = np.zeros(p)
        beta[cols] = rng.standard_normal(m) / np.sqrt(m)
        time = rng.integers(0, int(2.5 * n), n) / 8.0  # about a third of the rows share a time
        status = (rng.uniform(size=n) < 0.7).astype(np.float64)
        w = rng.integers(0, 17, n) / 8.0
        _COX[m] = dict(X=X, cols=cols, beta=beta, time=time, status=status, w=w, y=np.column_stack([time, status]))
    return _COX[m]


@pytest.mark.parametrize("ties", ["order", "breslow"])
@pytest.mark.parametrize("m", [1, 17])
def test_cox_meat_of_the_score_residuals(gpu, m, ties):
    cs = _cox_case(m)
    n = 300
    t = _dev(cs["X"])
    dref = coxdiagref.cox_diag_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["time"], cs["status"], cs["w"],
                                         ties, None, None, coxdiagref.device_depths(m))
    L = gpu.cox_diagnostics_device(t, cs["cols"], cs["beta"][cs["cols"]], cs["time"], cs["status"], weight=cs["w"],
                                   ties=ties, kinds=("score",))["score"]
    est = linear.PdasCox()
    est.p, est.beta, est.coef0 = cs["beta"].size, cs["beta"], 0.0
    for lab in (None, "random", "sorted"):
        labels = None if lab is None else _labels(gpu, lab, n)
        dd = sandwichref.device_depths(gpu, n, m, labels, intercept=False)
        ref = sandwichref.rows_reference(dref["score"], dref["score_bound"], labels, *dd)
        got = gpu.meat_device(L, np.arange(m), cluster=labels, intercept=False)
        what = "cox m=%d %s %s" % (m, ties, lab)
        sandwichref.check_meat(got, ref, what)
        assert got["n_clusters"] == (None if lab is None else ref["G"])
        assert (np.abs(got["sums"].astype(LD) - ref["sums"]) <= ref["sums_bound"]).all()
        # the estimator: device route against the NumPy route within the two bounds
        kind = "HC0" if lab is None else "HC1"
        dev = est.inference_survival(t, cs["y"], weight=cs["w"], ties=ties, cov_type=kind,
                                     cluster=None if labels is None else _dev(labels))
        host = est.inference_survival(cs["X"], cs["y"], weight=cs["w"], ties=ties, cov_type=kind, cluster=labels)
        href = coxdiagref.cox_diag_reference(cs["X"], cs["cols"], cs["beta"][cs["cols"]], cs["time"], cs["status"], cs["w"],
                                             ties, None, None, coxdiagref.host_depths(m))
        rh = sandwichref.rows_reference(href["score"], href["score_bound"], labels, *sandwichref.host_depths(n, labels))
        assert np.array_equal(dev["meat"], got["meat"])
        err = np.abs(dev["meat"].astype(LD) - host["meat"].astype(LD))
        print("%s: device - host %.3e against %.3e" % (what, float(err.max()), float(2 * np.maximum(
            ref["meat_bound"], rh["meat_bound"]).max())))
        assert (err <= 2 * np.maximum(ref["meat_bound"], rh["meat_bound"])).all()
        assert dev["n_clusters"] == host["n_clusters"] and dev["scale"] == host["scale"] and dev["cov_type"] == kind


@pytest.mark.parametrize("name", ["PdasLm", "PdasLogistic", "PdasPoisson"])
def test_estimator_inference_on_a_device_matrix_agrees_with_the_numpy_route(gpu, name):
    n, p, k = 400, 60, 4
    rng = np.random.default_rng(21)
    X = rng.standard_normal((n, p))
    truth = np.zeros(p)
    truth[rng.choice(p, k, replace=False)] = np.array([1.0, -1.0, 0.8, -0.8])
    eta = X @ truth + 0.2
    y = {"PdasLm": eta + rng.standard_normal(n) * (1 + np.abs(X[:, 0])),
         "PdasLogistic": (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))) * 1.0,
         "PdasPoisson": rng.poisson(np.exp(eta)) * 1.0}[name]
    w = rng.integers(1, 17, n) / 8.0
    labels = _labels(gpu, "random", n)
    est = getattr(linear, name)(sequence=list(range(1, 7)))
    Xd = _dev(X)
    est.fit(Xd, y)
    link = est._LINK[est.model_type_int]
    cols = np.nonzero(est.beta)[0]
    m, c0 = cols.size, float(np.ravel(est.coef0)[0])
    iref = inforef.information_reference(X, cols, est.beta[cols], c0, y, w, link,
                                         max(n, inforef.device_depth(gpu, n, m)))
    plain = est.inference(Xd, _dev(y), weight=w)
    assert set(plain) == set(est.inference(X, y, weight=w)) and "meat" not in plain
    for kind, lab in (("HC0", None), ("HC1", None), ("HC2", None), ("HC3", None), ("HC0", labels), ("HC1", labels)):
        dev = est.inference(Xd, _dev(y), weight=_dev(w), cov_type=kind, cluster=None if lab is None else _dev(lab))
        host = est.inference(X, y, weight=w, cov_type=kind, cluster=lab)
        # HC2 / HC3: each route factors ITS information, and R is data to the meat, so each route has its own reference,
        # built from its own R.  Two results that are each within their bound of their reference differ by at most the
        # two bounds plus the distance of the two references, which is formed here in longdouble (0 for HC0 / HC1).
        Rd = Rh = None
        if kind in ("HC2", "HC3"):
            Rd = capi.info_factor(gpu.information_device(Xd, cols, est.beta[cols], c0, _dev(y), link=link,
                                                         weight=_dev(w))["info"])[0]
            Rh = capi.info_factor(linear.bess_base._information_host(link, X[:, cols], est.beta[cols], c0, y, w)["info"])[0]
        rd = sandwichref.meat_reference(X, cols, est.beta[cols], c0, y, w, link, kind, Rd, lab,
                                        sandwichref.device_depths(gpu, n, m, lab))
        rh = sandwichref.meat_reference(X, cols, est.beta[cols], c0, y, w, link, kind, Rh, lab,
                                        sandwichref.host_depths(n, lab), host=True)
        what = "%s %s clustered=%s" % (name, kind, lab is not None)
        sandwichref.check_meat({"meat": dev["meat"]}, rd, what + " device")
        sandwichref.check_meat({"meat": host["meat"]}, rh, what + " host")
        gap = np.abs(rd["meat"] - rh["meat"])
        err = np.abs(dev["meat"].astype(LD) - host["meat"].astype(LD))
        print("%s: meat device - host %.3e against %.3e (of which the references differ by %.3e)" % (
            what, float(err.max()), float((rd["meat_bound"] + rh["meat_bound"] + gap).max()), float(gap.max())))
        assert (err <= rd["meat_bound"] + rh["meat_bound"] + gap).all()
        ses = []
        for tb, rf in ((dev, rd), (host, rh)):
            assert tb["positive_definite"] and tb["cov_type"] == kind and np.array_equal(tb["cols"], cols)
            cov, se, bdiag, bse, _ = sandwichref.covariance_reference(iref["info"], rf["meat"], tb["scale"],
                                                                      info_rel=iref["rel"], meat_bound=rf["meat_bound"])
            assert (np.abs(tb["se"].astype(LD) - se) <= bse).all(), what
            ses.append((se, bse))
        assert (np.abs(dev["se"] - host["se"]).astype(LD) <= ses[0][1] + ses[1][1] + np.abs(ses[0][0] - ses[1][0])).all()
        assert dev["n_clusters"] == host["n_clusters"] and dev["scale"] == host["scale"]
        assert np.array_equal(dev["coef"], host["coef"]) and dev["dof"] == host["dof"] == n - m - 1


def test_device_memory_is_given_back(gpu):
    n, m = 4097, 31
    pr = _problem("f64", n, m)
    t = _dev(pr["vals"])
    y, w, labels = pr["ys"]["logistic"], _dev(pr["w"]), _labels(gpu, "long", n)
    R, _ = _factor(pr, "logistic", y, pr["w"])
    before = gpu.process_counters()
    for kind, lab in (("HC0", None), ("HC3", None), ("HC1", labels)):
        _call(gpu, t, pr, "logistic", y, w, kind, lab, R)
        gpu.meat_device(t, pr["cols"], cluster=lab)
        c = gpu.process_counters()
        assert c["live_device_bytes"] == before["live_device_bytes"]
        assert c["live_pinned_bytes"] == before["live_pinned_bytes"]
