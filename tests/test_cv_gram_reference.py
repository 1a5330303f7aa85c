"""CPU: the check of tests/test_cv_gram_gpu.py bites, and the geometry it expects is stated here, not read from the library.

(1) fp64 NumPy forming X_m^T X_m[:, cols] -- directly, and as slab partials of the fold-major copy summed in the device's
order (cvgramref.gram_in_device_order) -- stays inside xprec.assert_gram_close's bound against the longdouble reference
of every row set, with the column norms and the row count of THAT row set, as the GPU file takes them.  The reference
arithmetic alone therefore does not need a wider bound on any of the small shapes.  Largest fraction of the bound used
(printed per case): 0.031 direct, 0.030 in the device's order.
(2) Three wrong Grams are rejected by the same call: the wrong fold left out, 64 rows (one slab's worth) of the fold
that should be left out included, one training row dropped.
(3) The pure-Python replica of the fold-major copy's geometry (cvgramref.fill_geometry) gives the values the issue states
for its cases (cvp_nsl = 2 and 3, cvp_rps = 128 for folds of 65/64/64, the refusal at 500/50/50), and every case of the
GPU file lands on the route its name says.

The design is xprec.design_large_mean with xprec.weights, normalised by xprec.normalize and rounded to fp64: fp64 columns
like the ones the library holds (the GPU file reads the library's own)."""
import numpy as np
import pytest

import cvgramref as C
import xprec

_designs = {}


def _design(n, p):
    if (n, p) not in _designs:
        X, y = xprec.design_large_mean(n, p)
        Xs = xprec.normalize(X, y, xprec.weights(n))[0].astype(np.float64)
        Xs.setflags(write=False)
        _designs[(n, p)] = Xs
    return _designs[(n, p)]


SMALL = [c for c in C.NEAR_EQUAL if c.p in (96, 257)] + C.PER_SET + C.UNEQUAL + C.REFUSED


def _norms(Xs, m):
    return np.sqrt((Xs[m] * Xs[m]).sum(axis=0))


def test_extended_precision_is_available():
    assert xprec.EXTENDED, "np.longdouble is not the x86 extended format here: the reference is no better than fp64"


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_fp64_numpy_stays_inside_the_bound_on_every_row_set(case):
    Xs = _design(case.n, case.p)
    fold, sizes = case.fold(), case.fold_sizes()
    S1, S2 = C.listed_columns(case.p)
    cols = np.union1d(S1, S2)
    # the device's order needs a geometry even where the library refuses the copy: the rule's values without the refusal
    nsl = max(1, (max(sizes) + 1023) // 2048)
    rps = ((max(sizes) + nsl - 1) // nsl + 63) // 64 * 64
    worst = [0.0, 0.0]
    for r, m in enumerate(C.masks(fold, case.K)):
        want = xprec.gram_columns(Xs, m, cols)
        norms = _norms(Xs, m)
        nr = int(m.sum())
        direct = Xs[m].T @ Xs[m][:, cols]
        device = C.gram_in_device_order(Xs, fold, case.K, nsl, rps, r, cols)
        what = "%s row set %d" % (case.id, r)
        worst[0] = max(worst[0], xprec.assert_gram_close(direct, want, norms[cols], norms, nr, what + ", direct"))
        worst[1] = max(worst[1], xprec.assert_gram_close(device, want, norms[cols], norms, nr, what + ", device order"))
    print("%s: %.4f of the bound (direct), %.4f (slab partials in the device's order)" % (case.id, worst[0], worst[1]))


CORRUPT = [c for c in SMALL if c.p == 96 or c.sizes is not None]


@pytest.mark.parametrize("case", CORRUPT, ids=lambda c: c.id)
def test_wrong_grams_are_rejected(case):
    Xs = _design(case.n, case.p)
    fold = case.fold()
    S1, S2 = C.listed_columns(case.p)
    cols = np.union1d(S1, S2)
    ms = C.masks(fold, case.K)
    for r in range(1, case.K + 1):
        m = ms[r]
        want = xprec.gram_columns(Xs, m, cols)
        norms = _norms(Xs, m)
        nr = int(m.sum())

        def check(G, what):
            return xprec.assert_gram_close(G, want, norms[cols], norms, nr, "%s row set %d: %s" % (case.id, r, what))

        check(Xs[m].T @ Xs[m][:, cols], "the right rows")
        other = ms[r % case.K + 1]  # the next fold left out instead
        with pytest.raises(AssertionError):
            check(Xs[other].T @ Xs[other][:, cols], "the wrong fold left out")
        extra = m.copy()
        extra[np.nonzero(~m)[0][:64]] = True  # (up to) one slab's worth of the fold that should be left out
        assert extra.sum() > m.sum()
        with pytest.raises(AssertionError):
            check(Xs[extra].T @ Xs[extra][:, cols], "64 rows of the left-out fold included")
        less = m.copy()
        less[np.nonzero(m)[0][nr // 2]] = False
        with pytest.raises(AssertionError):
            check(Xs[less].T @ Xs[less][:, cols], "one training row dropped")


def test_device_order_with_the_wrong_slabs_left_out_is_rejected():
    """The multiplication the small shapes never see: at 2 slabs per fold, leaving out slabs [r - 1, r) instead of
    [2 (r - 1), 2 r) -- ex_lo / ex_hi without the factor cvp_nsl -- is outside the bound.  (A reduced replica of the
    two-slab cases: folds of 70 rows cut into 2 slabs of 64, which the library itself would not do below 3073 rows.)"""
    n, p, K, nsl, rps = 210, 96, 3, 2, 64
    Xs = _design(n, p)
    fold = C.folds_of_sizes(n, (70, 70, 70))
    cols = C.listed_columns(p)[0]
    for r, m in enumerate(C.masks(fold, K)):
        want = xprec.gram_columns(Xs, m, cols)
        norms = _norms(Xs, m)
        args = (norms[cols], norms, int(m.sum()), "two slabs per fold, row set %d" % r)
        xprec.assert_gram_close(C.gram_in_device_order(Xs, fold, K, nsl, rps, r, cols), want, *args)
        if r >= 1:
            with pytest.raises(AssertionError):
                xprec.assert_gram_close(C.gram_in_device_order(Xs, fold, K, nsl, rps, r, cols, skip=(r - 1, r)), want, *args)


def test_geometry_replica_states_the_issues_values():
    g = C.fill_geometry
    assert g(130, (60, 40, 30)) == {"shared": True, "cvp_nsl": 1, "cvp_rps": 64, "copy_rows": 192}
    assert g(193, (65, 64, 64)) == {"shared": True, "cvp_nsl": 1, "cvp_rps": 128, "copy_rows": 384}
    assert g(600, (250, 200, 150)) == {"shared": True, "cvp_nsl": 1, "cvp_rps": 256, "copy_rows": 768}
    assert g(6145, (3073, 3072)) == {"shared": True, "cvp_nsl": 2, "cvp_rps": 1600, "copy_rows": 6400}
    assert g(10241, (5121, 5120)) == {"shared": True, "cvp_nsl": 3, "cvp_rps": 1728, "copy_rows": 10368}
    assert g(9217, (3073, 3072, 3072)) == {"shared": True, "cvp_nsl": 2, "cvp_rps": 1600, "copy_rows": 9600}
    # 3 x 512 = 1536 rows against 640 padded rows of X
    assert g(600, (500, 50, 50)) == {"shared": False, "cvp_nsl": 0, "cvp_rps": 0, "copy_rows": 0}
    # the boundaries of the slab count: one slab up to 3072 rows, two up to 5120
    assert g(6144, (3072, 3072))["cvp_nsl"] == 1 and g(10240, (5120, 5120))["cvp_nsl"] == 2
    # exactly 1.5 times the rows of X is still accepted (384 against 256)
    assert C.session_rows(193) == 256 and C.session_rows(1100) == 1280 and C.session_rows(6145) == 7168


def test_every_case_lands_on_the_route_its_name_says():
    for c in C.SHARED_CASES + C.HOOK:
        got = c.geometry()
        assert got["shared"] == (c.route in ("sets", "per-set")), c.id
        if c.route == "sets":
            assert c.K + 1 <= 9, c.id
        if c.route == "per-set":
            assert c.K + 1 > 9, c.id
        for k, v in (c.want or {}).items():
            assert got[k] == v, (c.id, k, got[k], v)
        if c.sizes is not None:
            assert c.fold_sizes() == list(c.sizes), c.id
        assert min(c.n - s for s in c.fold_sizes()) > C.K40, c.id + ": a 40-column model needs more training rows"
    reached = {c.route for c in C.SHARED_CASES}
    assert reached == {"sets", "per-set", "refused"}
    assert {c.geometry()["cvp_nsl"] for c in C.MULTI_SLAB} == {2, 3}
