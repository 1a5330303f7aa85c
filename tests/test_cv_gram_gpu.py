"""GPU: the Gram columns that the row sets of a cross-validation hold cached, entry by entry against np.longdouble.

What is read.  Session.cov_cache_columns(r, cols) (bessx_session_cov_cache_columns) copies the columns row set r holds
right now -- r = 0 all rows, r = k + 1 the training rows of fold k -- out of the OWNER's cache: the fold contexts of the
side-by-side chains borrow the session's caches (fold_ctx_create copies the cov vector), so one read serves every fit of
the row set, wherever it ran.  Session.cv_fill_geometry() says whether the folds share their fills and how the
fold-major copy is cut; the expected answer comes from the pure-Python replica in tests/cvgramref.py, whose values
tests/test_cv_gram_reference.py pins to the figures of the change's issue.

Reference and bound.  The design is xprec.design_large_mean with xprec.weights (as tests/test_panel_shapes_gpu.py); the
reference, xprec.gram_columns in longdouble, reads the library's own fp64 columns (op_normalize) under the row set's
mask; the bound is xprec.assert_gram_close's 32 sqrt(n) u |x_j| |x_a| with the column norms over the rows of the row set
and n its row count.  tests/test_cv_gram_reference.py shows on the CPU that fp64 NumPy uses at most 0.031 of it on these
shapes (0.030 summing slab partials in the device's order) and that a wrong fold, 64 foreign rows or one dropped row
fall outside it.  The response is built from the first listed model (40 columns) so that a fit started from it stays on
it: which launches a fit makes is then known, and every column a row set reports cached is compared -- the listed ones are
required, the ones a fit or a path added on its own (selected or speculative) are held to the same bound.

Getting columns cached.  s.fit(40, 0, fold, init) on a cold cache lists the 40 columns of the initial model: 64 entries,
24 of them -1, one two-group launch; a second fit whose model shares 8 of them lists 32: one group.  Under shared fills
both enter all K + 1 caches at once (first fit on fold 0, second on fold K - 1); under masked fills only the fitted fold's.

Cases (tests/cvgramref.py), named by what they reach; each asserts the route from cv_fill_geometry() and the counters:
  * near-equal folds, K = 2, 3, 4, 8 at n in {130, 600, 1100}, p in {96, 130, 257}: shared fills, all row sets in one
    k_cov_reduce_sets launch (K + 1 <= 9).  K = 8 at n = 130 and n = 600 is NOT shared: 8 folds of 16-18 (75) rows pad to
    8 slabs of 64 (128) rows, more than 1.5 times the session's 256 (640) rows, and set_cv refuses the copy -- these four
    shapes run, and are held to the bound, on masked fills.  K = 8 at n = 1100 is the nine-row-set launch;
  * K + 1 > 9, one k_cov_reduce + k_cov_compact per row set: K = 10 at n = 600; K = 9 at n = 600 is refused by the same
    rule (folds of 66-72 rows, slabs of 128), so K = 9 at n = 576 (folds of exactly 64 rows) is added for the threshold;
    (which reduce runs is decided by K + 1 > 9 alone in enqueue_cov_fill; no counter tells them apart, the case asserts K)
  * unequal and short folds, still shared: 60/40/30 (every fold under one 64-row slab), 65/64/64 (cvp_rps = 128, half of
    every segment padding), 250/200/150;
  * more than one slab per fold -- the only shapes at which ex_lo / ex_hi are multiplied by something other than 1:
    3073/3072 (cvp_nsl = 2), 5121/5120 (cvp_nsl = 3), 3073/3072/3072 (the middle fold's exclusion [2, 4) has slabs on
    both sides);
  * the refusal: 500/50/50 at n = 600 (a copy of 1536 rows against 640): masked fills, every fold fitted and compared;
  * masked fills by the test hook cv_shared=0: a fit on fold 1 caches into row set 2 and nowhere else.
Relations: the export is bitwise the same after reset_caches() and the same fits; every row set's block G_r[cols, cols]
against its transpose (twice the bound; whether it is bitwise symmetric is recorded below); the caches as a traced and
an untraced golden-section CV path leave them (the untraced one runs the folds side by side on their own streams).

Measured maxima (MI355X), fraction of the bound used, per route:
  shared fills, k_cov_reduce_sets (K + 1 <= 9, one slab per fold)            0.025
  shared fills, one reduce per row set (K = 9 at n = 576, K = 10)            0.0047
  shared fills, cvp_nsl = 2 and 3                                            0.011
  masked fills, copy refused by the 1.5 x rule (500/50/50; K = 8, 9 above)   0.038
  masked fills by the hook cv_shared=0                                       0.027
  caches a CV path leaves, traced and untraced (same figures)                0.011 shared, 0.0044 per-set, 0.010 refused
  No case needed more than 4 % of the bound, the CPU stand-in needs 3 %: no wrong entry, no bug found in the ex_lo / ex_hi
  arithmetic, the padding rows of the copy or the slot maps under the refusal.
  That the check bites on the device too: in a local build with the factor cvp_nsl taken out of ex_lo / ex_hi the three
  shapes with more than one slab per fold fail (entries off by 1e12 times the bound) and the one-slab shapes pass.
Symmetry: the block G_r[cols, cols] was BITWISE symmetric in every row set of every case, shared and masked, after fits
and after paths (as the unmasked prefill route is); the test asserts twice the bound and prints the finding.
Launches: the first fit made exactly one two-group launch in all 104 fits of that kind; the second 1 to 6 one-group
launches (its own 32 missing columns, then what it selected on the way back to the first model).
Cost: the file (66 tests) takes 12.1 s where tests/test_cov_gpu.py (39 tests) takes 8.4 s in the same GPU run; no case
takes more than 0.7 s, the slowest being K = 8 at n = 1100, p = 257 (nine longdouble references) and the three shapes
with more than one slab per fold (6145 to 10241 rows).
"""
import time

import numpy as np
import pytest

import cvgramref as C
import xprec
from helpers import hooks

pytestmark = pytest.mark.gpu

REPORT = {}      # route -> largest fraction of the bound seen
ASYMMETRIC = {}  # route -> row sets whose exported block was not bitwise symmetric
_designs = {}
_refs = {}


def _note(route, value):
    REPORT[route] = max(REPORT.get(route, 0.0), float(value))


@pytest.fixture(scope="module")
def ref(gpu):
    if not xprec.EXTENDED:
        pytest.skip("np.longdouble is not the x86 extended format on this host: no extended-precision reference")
    t0 = time.time()
    yield gpu
    for k in sorted(REPORT):  # (the source of the table in the header; shown with -s)
        print("MEASURED %-44s %.4f of the bound; row sets not bitwise symmetric: %d" % (k, REPORT[k], ASYMMETRIC.get(k, 0)))
    print("MEASURED wall time of this file %.1f s" % (time.time() - t0))


def _design(gpu, n, p):
    """Design, response, weights, the library's own normalised columns and response, the two listed models."""
    if (n, p) not in _designs:
        X, _ = xprec.design_large_mean(n, p)
        w = xprec.weights(n)
        S1, S2 = C.listed_columns(p)
        rng = np.random.Generator(np.random.PCG64(7 * n + p))
        Z = (X[:, S1] - 1e6) / 10.0 ** (S1 % 7 - 3.0)
        y = Z @ (rng.uniform(1.0, 2.0, S1.size) * rng.choice([-1.0, 1.0], S1.size)) + 0.05 * rng.standard_normal(n) + 3.0
        Xs, ys = gpu.op_normalize(X, y, w, 1, True, True)[:2]
        Xs.setflags(write=False)
        _designs[(n, p)] = (X, y, w, Xs, ys, S1, S2)
    return _designs[(n, p)]


def _reference(case, Xs, r, mask, cols):
    key = (case.id, r, cols.tobytes())
    if key not in _refs:
        want = xprec.gram_columns(Xs, mask, cols)
        want.setflags(write=False)
        _refs[key] = want
    return _refs[key]


def _start(Xs, ys, mask, S):
    return np.linalg.lstsq(Xs[mask][:, S], ys[mask], rcond=None)[0]


def _delta(after, before):
    return {k: after[k] - before[k] for k in ("passes_over_X", "panel_launches_one_group", "panel_launches_two_groups")}


def _export(s, r, p):
    G, hit = s.cov_cache_columns(r, np.arange(p, dtype=np.int32))
    assert np.isfinite(G[:, hit]).all() and np.isnan(G[:, ~hit]).all()
    return G, hit


def _check_row_set(s, case, Xs, r, mask, must_have, route, what):
    """Every column row set r reports cached against the longdouble reference under ITS mask; the listed ones required.
    Returns the cached columns."""
    p = Xs.shape[1]
    G, hit = _export(s, r, p)
    assert hit[must_have].all(), "%s row set %d: listed columns %s are not cached" % (what, r, must_have[~hit[must_have]])
    cols = np.nonzero(hit)[0]
    got = G[:, cols]
    norms = np.sqrt((Xs[mask] * Xs[mask]).sum(axis=0))
    nr = int(mask.sum())
    label = "%s, row set %d (%d rows, %d columns cached)" % (what, r, nr, cols.size)
    f = xprec.assert_gram_close(got, _reference(case, Xs, r, mask, cols), norms[cols], norms, nr, label)
    sub = got[cols, :]
    xprec.assert_gram_close(sub, sub.T, norms[cols], norms[cols], nr, label + ": block against its transpose", scale=2.0)
    sym = bool(np.array_equal(sub, sub.T))
    if not sym:
        ASYMMETRIC[route] = ASYMMETRIC.get(route, 0) + 1
    _note(route, f)
    print("%s: %.4f of the bound, block bitwise symmetric: %s" % (label, f, sym))
    return cols


def _session(gpu, case):
    X, y, w, Xs, ys, S1, S2 = _design(gpu, case.n, case.p)
    s = gpu.Session(X, y, weight=w, score_mode=2)
    return s, Xs, ys, S1, S2


def _route_label(case, geo):
    if case.route in ("sets", "per-set"):
        return "shared, cvp_nsl > 1" if geo["cvp_nsl"] > 1 else ("shared, _sets reduce" if case.K + 1 <= 9 else "shared, per-set reduce")
    return "masked (copy refused)" if case.route == "refused" else "masked (hook)"


def _two_fits(s, Xs, ys, ms, S1, S2, f1, f2):
    """The 40-column fit from S1 on fold f1, then the fit from S2 (8 columns shared) on fold f2; their launch counts."""
    c0 = s.counters()
    s.fit(C.K40, 0.0, f1, init_idx=S1, init_val=_start(Xs, ys, ms[f1 + 1], S1))
    c1 = s.counters()
    s.fit(C.K40, 0.0, f2, init_idx=S2, init_val=_start(Xs, ys, ms[f2 + 1], S2))
    return _delta(c1, c0), _delta(s.counters(), c1)


def _assert_two_fills(d1, d2, what):
    # cold cache, a fit that stays on its initial model: its 40 columns are ONE padded two-group launch and nothing else;
    # of the second model's 40 columns 32 are missing -- a one-group list -- and what the fit selects on its way back to
    # the first model comes in further one-group fills
    assert d1 == {"passes_over_X": 2, "panel_launches_one_group": 0, "panel_launches_two_groups": 1}, (what, d1)
    assert d2["panel_launches_one_group"] >= 1 and d2["panel_launches_two_groups"] == 0 and d2["passes_over_X"] >= 1, (what, d2)


def _assert_geometry(s, case):
    geo = s.cv_fill_geometry()
    assert geo == case.geometry(), "%s: the library lays the copy out as %s, the rule says %s" % (case.id, geo, case.geometry())
    for k, v in (case.want or {}).items():
        assert geo[k] == v, (case.id, k, geo[k], v)
    assert geo["shared"] == (case.route in ("sets", "per-set")), (case.id, geo)
    if case.route == "sets":
        assert case.K + 1 <= 9
    if case.route == "per-set":
        assert case.K + 1 > 9
    return geo


@pytest.mark.parametrize("case", C.SHARED_CASES, ids=lambda c: c.id)
def test_every_row_set_against_its_own_masked_reference(ref, case):
    gpu = ref
    s, Xs, ys, S1, S2 = _session(gpu, case)
    fold, K, p = case.fold(), case.K, case.p
    ms = C.masks(fold, K)
    both = np.union1d(S1, S2)
    with s:
        s.set_cv(K, fold)
        geo = _assert_geometry(s, case)
        route = _route_label(case, geo)
        s.enable_kernel_timing(True)
        if geo["shared"]:
            c0 = s.counters()
            s.fit(C.K40, 0.0, 0, init_idx=S1, init_val=_start(Xs, ys, ms[1], S1))
            c1 = s.counters()
            for r in range(K + 1):  # one fill, on fold 0's behalf, entered ALL caches
                assert _export(s, r, p)[1][S1].all(), "%s: row set %d lacks the first fit's columns" % (case.id, r)
            s.fit(C.K40, 0.0, K - 1, init_idx=S2, init_val=_start(Xs, ys, ms[K], S2))
            d1, d2 = _delta(c1, c0), _delta(s.counters(), c1)
            print("%s: %s; first fit %s, second fit %s" % (case.id, geo, d1, d2))
            _assert_two_fills(d1, d2, case.id)
            sets = [_check_row_set(s, case, Xs, r, ms[r], both, route, case.id) for r in range(K + 1)]
            for c in sets[1:]:
                assert np.array_equal(c, sets[0]), "row sets that share their fills report different cached columns"
        else:
            # the copy was refused: every fold's cache is its own, filled by masked passes over X
            for k in range(K):
                assert not _export(s, k + 1, p)[1].any(), "%s: fold %d holds columns before its first fit" % (case.id, k)
                d1, d2 = _two_fits(s, Xs, ys, ms, S1, S2, k, k)
                print("%s fold %d: first fit %s, second fit %s" % (case.id, k, d1, d2))
                _assert_two_fills(d1, d2, "%s fold %d" % (case.id, k))
                _check_row_set(s, case, Xs, k + 1, ms[k + 1], both, route, case.id)
            assert not _export(s, 0, p)[1].any(), "a fold's masked fill reached the all-rows cache"


@pytest.mark.parametrize("case", C.HOOK, ids=lambda c: c.id)
def test_masked_fills_cache_into_the_fitted_fold_only(ref, monkeypatch, case):
    gpu = ref
    hooks(monkeypatch, cv_shared="0")
    s, Xs, ys, S1, S2 = _session(gpu, case)
    fold, K, p = case.fold(), case.K, case.p
    assert C.fill_geometry(case.n, case.fold_sizes())["shared"], "without the hook this shape shares its fills"
    ms = C.masks(fold, K)
    with s:
        s.set_cv(K, fold)
        _assert_geometry(s, case)
        s.enable_kernel_timing(True)
        d1, d2 = _two_fits(s, Xs, ys, ms, S1, S2, 1, 1)
        print("%s: first fit %s, second fit %s" % (case.id, d1, d2))
        _assert_two_fills(d1, d2, case.id)
        for r in (0, 1, 3):
            assert not _export(s, r, p)[1].any(), "a fit on fold 1 cached columns in row set %d" % r
        _check_row_set(s, case, Xs, 2, ms[2], np.union1d(S1, S2), "masked (hook)", case.id)


def _by_id(cases, name, **kw):
    got = [c for c in cases if c.name == name and all(getattr(c, k) == v for k, v in kw.items())]
    assert len(got) == 1, (name, kw)
    return got[0]


REPEAT = [_by_id(C.NEAR_EQUAL, "near-equal", n=600, p=130, K=3), _by_id(C.NEAR_EQUAL, "near-equal", n=1100, p=257, K=8),
          _by_id(C.PER_SET, "per-set-reduce", n=600, K=10), _by_id(C.UNEQUAL, "one-row-over-a-slab"),
          _by_id(C.MULTI_SLAB, "two-slabs-middle-fold")]


@pytest.mark.parametrize("case", REPEAT, ids=lambda c: c.id)
def test_shared_fills_repeat_bit_for_bit(ref, case):
    """reset_caches() and the same fits: the same session exports the same bits (the summation order is fixed)."""
    gpu = ref
    s, Xs, ys, S1, S2 = _session(gpu, case)
    fold, K, p = case.fold(), case.K, case.p
    ms = C.masks(fold, K)
    with s:
        s.set_cv(K, fold)
        assert _assert_geometry(s, case)["shared"]
        runs = []
        for _ in range(2):
            s.reset_caches()
            assert not _export(s, 0, p)[1].any() and not _export(s, K, p)[1].any()
            _two_fits(s, Xs, ys, ms, S1, S2, 0, K - 1)
            runs.append([_export(s, r, p) for r in range(K + 1)])
        for r in range(K + 1):
            (G0, h0), (G1, h1) = runs[0][r], runs[1][r]
            assert h0[np.union1d(S1, S2)].all() and np.array_equal(h0, h1)
            assert np.array_equal(G0[:, h0], G1[:, h1]), "%s row set %d: the second run's columns differ" % (case.id, r)


PATHS = [_by_id(C.NEAR_EQUAL, "near-equal", n=600, p=130, K=4), _by_id(C.PER_SET, "per-set-reduce", n=600, K=10),
         _by_id(C.UNEQUAL, "one-row-over-a-slab"), _by_id(C.REFUSED, "copy-refused")]


@pytest.mark.parametrize("traced", (True, False), ids=("traced", "untraced"))
@pytest.mark.parametrize("case", PATHS, ids=lambda c: c.id)
def test_caches_as_a_cv_path_leaves_them(ref, case, traced):
    """A golden-section CV path over 1..12 columns: whatever it left cached (selected and speculative columns) in every
    row set is inside the bound.  Untraced, folds of up to 8 run side by side in their own contexts."""
    gpu = ref
    s, Xs, ys, S1, S2 = _session(gpu, case)
    fold, K, p = case.fold(), case.K, case.p
    ms = C.masks(fold, K)
    with s:
        s.set_cv(K, fold)
        geo = _assert_geometry(s, case)
        route = _route_label(case, geo) + (", traced path" if traced else ", untraced path")
        s.trace_enable(traced)
        out = s.gs_path(1, 12, ic_type=3, is_cv=True)
        print("%s: %s, fold contexts %d, side-by-side rounds %d" % (case.id, geo, s.counters()["cv_fold_contexts"],
                                                                     s.counters()["cv_side_by_side_rounds"]))
        assert out["n_candidates"] >= 3
        if not traced and geo["shared"] and K <= 8:
            assert s.counters()["cv_fold_contexts"] == K and s.counters()["cv_side_by_side_rounds"] > 0
        none = np.zeros(0, dtype=np.int64)  # (which columns a path leaves is its own business: all it left are compared)
        for r in range(K + 1):
            # every candidate is fitted on all rows and on every fold's training rows: no row set stays empty
            cols = _check_row_set(s, case, Xs, r, ms[r], none, route, case.id)
            assert cols.size >= 1, "%s: row set %d is empty after a CV path" % (case.id, r)


def test_the_export_reads_and_changes_nothing(ref):
    """Without folds the export is the prefill route's, bit for bit; it leaves counters and the slot map alone; it
    refuses what it cannot serve."""
    gpu = ref
    n, p = 600, 130
    X, y, w, Xs, ys, S1, S2 = _design(gpu, n, p)
    cols = ((np.arange(64) * 29 + 7) % p).astype(np.int32)
    with gpu.Session(X, y, weight=w, score_mode=2) as s:
        assert s.cv_fill_geometry() == {"shared": False, "cvp_nsl": 0, "cvp_rps": 0, "copy_rows": 0}
        s.cov_prefill_begin(cols)
        s.cov_prefill_compute(0, 2)
        want = s.cov_prefill_export(0, 2).reshape(64, p).T
        s.cov_prefill_end()
        before, slots = s.counters(), s.cov_state()[1]
        G, hit = s.cov_cache_columns(0, np.arange(p, dtype=np.int32))
        assert np.array_equal(np.nonzero(hit)[0], np.sort(cols)) and np.array_equal(G[:, cols], want)
        G2, hit2 = s.cov_cache_columns(0, cols[::-1])  # (any order, any subset)
        assert hit2.all() and np.array_equal(G2, want[:, ::-1])
        assert s.counters() == before and np.array_equal(s.cov_state()[1], slots)
        for bad_set, bad_cols in ((1, cols), (-1, cols), (0, [p]), (0, [-1])):
            with pytest.raises(gpu.BessxError) as e:
                s.cov_cache_columns(bad_set, bad_cols)
            assert e.value.code == 1  # BESSX_ERR_ARG
        s.set_cv(3, C.folds_of_sizes(n, (250, 200, 150)))
        assert s.cov_cache_columns(3, cols)[1].sum() == 0  # (set_cv starts the shared caches from empty)
        with pytest.raises(gpu.BessxError) as e:
            s.cov_cache_columns(4, cols)
        assert e.value.code == 1
    with gpu.Session(X, y, weight=w, score_mode=1) as s:  # the streaming form has no Gram column cache
        with pytest.raises(gpu.BessxError) as e:
            s.cov_cache_columns(0, cols)
        assert e.value.code == 3  # BESSX_ERR_UNSUPPORTED
        assert s.cv_fill_geometry()["shared"] is False
