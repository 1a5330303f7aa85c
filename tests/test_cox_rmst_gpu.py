"""Restricted mean and quantile survival times on an X already in GPU memory (bessx_cox_survtime_device,
bess_amd/csrc/bessx_k_coxrmst.hip) against NumPy in np.longdouble on the host copy of the same values.  The bounds are
derived in tests/coxrmstref.py; every check prints error against bound, and every case that is not marked adversarial also
asserts that the bound itself is at most 1e-9 relative.  The problem is that of tests/test_cox_surv_gpu.py (4099 rows,
P = 80); the baseline is the longdouble reference's over all 4099 rows and the calls are made on the first n rows.  The
shapes are the smallest that reach every path: the 512-row tiles of the partial kernel (one and two rows per thread), the
256-row workgroups of the finish kernel, pieces of 1, SL - 1 and SL segments, several pieces, a cut on a piece boundary,
and more pieces than one chunk of rows may have partials for.

Bits across layouts: e is section 2f's predictor pass, used as it is so that every term is the element
cox_survival_device writes (test_the_terms_are_those_of_the_curve_kernel).  That pass adds the support's products in one
order for a row-contiguous X and in another for the other layouts (on the MI355X the RMST of a row then differs by a few
units in the last place between the two at m = 3).  So the tests ask for equal bits where e has them: every fp64 layout
for m <= 1, the layouts that share the pass's route for every m, and float32 against the float64 X of the same widened
values under either route -- as tests/test_cox_band_gpu.py does for the bands."""
import ctypes

import numpy as np
import pytest

import coxrmstref
import coxsurvref
import evalref
from bess_amd import linear, synth
from test_cox_surv_gpu import LAYOUTS, P, _bits, _dev, _problem, _view

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
U = evalref.U
NMAX = 1025
NS = [1, 2, 255, 256, 257, 513, 1025]
QS = np.array([0.1, 0.25, 0.5, 0.75, 0.9])
_REFS = {}


def _case(m, f32=False):
    """The problem with m support columns: the widened values, eta of the first NMAX rows, the baseline of all rows."""
    key = ("case", m, f32)
    if key not in _REFS:
        X, cols, B, time, status = _problem(4099, m)
        vals = X.astype(np.float32).astype(np.float64) if f32 else X
        eta, delta = evalref.eta_reference(vals, cols, np.asarray(B).reshape(-1, 1), [0.0])
        base = coxsurvref.baseline_reference(eta[:, 0], delta[:, 0], time, status, None)
        bt, bh = base["times"], np.asarray(base["cumhaz"], dtype=np.float64)
        assert 2400 <= bt.size <= 2560 and (np.diff(bh) >= 0).all()
        tau = np.array([np.quantile(time, 0.1), np.quantile(time, 0.5), np.quantile(time, 0.9), 1.5 * time.max()])
        _REFS[key] = dict(X=X, cols=cols, B=B, time=time, eta=eta[:NMAX, 0], delta=delta[:NMAX, 0], bt=bt, bh=bh, tau=tau)
    return _REFS[key]


def _rmst_ref(gpu, c, bt, bh, tau, rows=slice(None), adversarial=False):
    hs, wd, cut = gpu.rmst_segments(bt, bh, tau)
    return coxrmstref.rmst_reference(c["eta"][rows], c["delta"][rows], hs, wd, cut, adversarial=adversarial)


def _first(ref, n):
    return {k: v[:n] for k, v in ref.items()}


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


# ----------------------------------------------------------------------------------------------------------------
# edges
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 3, 70])
def test_row_tile_edges_for_every_layout_and_support(gpu, m):
    first = {}
    for layout in LAYOUTS:
        f32 = layout == "f32 row-major"
        c = _case(m, f32)
        bt, bh, tau = c["bt"], c["bh"], c["tau"]
        if "ref" not in c:  # (once per set of widened values)
            c["ref"] = _rmst_ref(gpu, c, bt, bh, tau)
            c["qref"] = coxrmstref.quantile_reference(c["eta"], c["delta"], bh, gpu.survival_levels(QS))
        ref, qref = c["ref"], c["qref"]
        if m > 0:  # (the +inf branch: rows that never reach q = 0.9)
            assert 0.3 <= float((qref["index"][:, -1] < bt.size).mean()) <= 0.9
        assert f32 or not qref["excused"].any()  # (the reference excuses none of the 5125 pairs of the fp64 values)
        for n in NS:
            t, _ = _view(c["X"][:n], layout)
            got = gpu.cox_survival_times_device(t, c["cols"], c["B"], bt, bh, tau=tau, q=QS)
            assert set(got) == {"rmst", "quantile"} and got["rmst"].is_cuda and tuple(got["rmst"].shape) == (n, 4)
            what = "n=%d m=%d %s" % (n, m, layout)
            coxrmstref.check_rmst(_np(got["rmst"]), _first(ref, n), what)
            coxrmstref.check_quantiles(_np(got["quantile"]), _first(qref, n), bt, what)
            # Equal widened values: the same bits wherever e has them.  e is section 2f's predictor pass as it is, which
            # adds the support's products in one order for a row-contiguous X and in another for the other layouts: every
            # fp64 layout agrees up to m = 1 (no sum), the layouts that share the pass's route agree for every m.
            group = "fp64" if m <= 1 else {"f64 column-major": "by rows", "strided": "by rows"}.get(layout)
            if not f32 and group is not None:
                keep = first.setdefault((group, n), (_bits(got["rmst"]), _bits(got["quantile"])))
                assert np.array_equal(_bits(got["rmst"]), keep[0]) and np.array_equal(_bits(got["quantile"]), keep[1]), what
        only = gpu.cox_survival_times_device(t, c["cols"], c["B"], bt, bh, tau=tau[:1])  # T = 1, the RMST part alone
        assert set(only) == {"rmst"} and np.array_equal(_bits(only["rmst"]), _bits(got["rmst"][:, :1]))
        only = gpu.cox_survival_times_device(t, c["cols"], c["B"], bt, bh, q=[0.5])  # the quantile part alone
        assert set(only) == {"quantile"} and np.array_equal(_bits(only["quantile"]), _bits(got["quantile"][:, 2:3]))


def test_piece_edges_with_truncated_baselines_and_a_cut_on_a_piece_boundary(gpu):
    c = _case(3)
    n = 257
    t = _dev(c["X"][:n])
    SL = gpu.cox_survtime_workspace(n, [1])["slab"]
    beyond = 1.5 * c["time"].max()
    for K, pieces in ((1, 1), (SL - 1, 1), (SL, 1), (SL + 1, 2), (2 * SL + 1, 3), (5 * SL + 3, 6)):
        bt, bh = c["bt"][:K - 1], c["bh"][:K - 1]  # K - 1 base times and one horizon beyond them: K segments
        hs, wd, cut = gpu.rmst_segments(bt, bh, [beyond])
        assert hs.size == K and cut.tolist() == [K] and gpu.cox_survtime_workspace(n, cut)["pieces"] == pieces
        got = gpu.cox_survival_times_device(t, c["cols"], c["B"], bt, bh, tau=[beyond])["rmst"]
        coxrmstref.check_rmst(_np(got), _rmst_ref(gpu, c, bt, bh, [beyond], slice(0, n)), "K=%d, T=1" % K)
    bt, bh = c["bt"][:3 * SL], c["bh"][:3 * SL]
    # T = 7: cuts at SL (a piece boundary exactly), SL + 1, 2 SL - 1, 2 SL, 0, a repeat, and everything
    tau = np.array([bt[SL - 1], bt[SL], bt[2 * SL - 2], bt[2 * SL - 1], 0.0, bt[SL], beyond])
    hs, wd, cut = gpu.rmst_segments(bt, bh, tau)
    assert cut.tolist() == [SL, SL + 1, 2 * SL - 1, 2 * SL, 0, SL + 1, 3 * SL + 1]
    assert gpu.cox_survtime_workspace(n, cut)["pieces"] == 6  # SL, 1, SL - 2, 1, SL, 1
    got = _np(gpu.cox_survival_times_device(t, c["cols"], c["B"], bt, bh, tau=tau)["rmst"])
    coxrmstref.check_rmst(got, _rmst_ref(gpu, c, bt, bh, tau, slice(0, n)), "T=7, a cut on a piece boundary")
    assert (got[:, 4] == 0.0).all() and np.array_equal(_bits(got[:, 1]), _bits(got[:, 5]))


def test_more_pieces_than_one_chunk_of_rows_may_hold(gpu):
    """20000 horizons at the 20000 times of a synthetic baseline: 20000 pieces, so that a chunk is 512 rows and n = 600
    takes two chunks.  The rows either side of the chunk boundary against the reference, and against an n = 1 call."""
    J, n, m = 20000, 600, 3
    c = _case(m)
    rng = np.random.default_rng(17)
    bt, bh = np.cumsum(rng.uniform(0.5, 1.5, J)) / J * 3.0, np.cumsum(rng.uniform(0.0, 2.0, J)) / J * 2.0
    hs, wd, cut = gpu.rmst_segments(bt, bh, bt)
    w = gpu.cox_survtime_workspace(n, cut)
    assert w["pieces"] == J and w["rows_per_chunk"] == 512 < n
    t = _dev(c["X"][:n])
    before = gpu.process_counters()
    got = gpu.cox_survival_times_device(t, c["cols"], c["B"], bt, bh, tau=bt)["rmst"]
    assert gpu.process_counters()["live_device_bytes"] == before["live_device_bytes"]  # (the partials are released)
    rows = np.array([0, 511, 512, 599])
    ref = coxrmstref.rmst_reference(c["eta"][rows], c["delta"][rows], hs, wd, cut)
    coxrmstref.check_rmst(_np(got[rows]), ref, "two chunks of rows")
    assert bool((got[:, 1:] >= got[:, :-1]).all())
    for i in (511, 512, 599):
        alone = gpu.cox_survival_times_device(t[i:i + 1], c["cols"], c["B"], bt, bh, tau=bt)["rmst"]
        assert np.array_equal(_bits(alone), _bits(got[i:i + 1])), i


# ----------------------------------------------------------------------------------------------------------------
# horizons, monotonicity, terms, bits
# ----------------------------------------------------------------------------------------------------------------
def test_horizons_at_before_and_beyond_the_event_times(gpu):
    c = _case(3)
    n, bt, bh = 513, c["bt"], c["bh"]
    t = _dev(c["X"][:n])
    call = lambda tau, b=(bt, bh): _np(gpu.cox_survival_times_device(t, c["cols"], c["B"], b[0], b[1], tau=tau)["rmst"])
    assert (call([0.0]) == 0.0).all()
    early = 0.5 * bt[0]
    assert (call([early]) == early).all() and (call([bt[0]]) == bt[0]).all()  # S = 1 up to and at the first event time
    tau = np.array([bt[700], 0.0, bt[-1] + 2.0, bt[5], bt[700], early, bt[-1], bt[-1] + 2.0, 0.5 * (bt[9] + bt[10])])
    got = call(tau)
    coxrmstref.check_rmst(got, _rmst_ref(gpu, c, bt, bh, tau, slice(0, n)), "horizons")
    distinct = np.unique(tau)
    want = call(distinct)  # unsorted and repeated: column for column the bits of the sorted distinct call
    assert np.array_equal(_bits(got), _bits(want[:, np.searchsorted(distinct, tau)]))
    last = _rmst_ref(gpu, c, bt, bh, [bt[-1], bt[-1] + 2.0], slice(0, n))["value"]  # the curve keeps its last value
    assert np.allclose(np.asarray(last[:, 1] - last[:, 0], dtype=np.float64),
                       2.0 * np.exp(-bh[-1] * np.exp(np.asarray(c["eta"][:n], dtype=np.float64))), rtol=1e-12)
    none = (np.zeros(0), np.zeros(0))  # J = 0: S = 1 everywhere
    got = gpu.cox_survival_times_device(t, c["cols"], c["B"], none[0], none[1], tau=[2.5, 0.0, 7.0], q=[0.5, 0.9])
    assert (_np(got["rmst"]) == np.array([2.5, 0.0, 7.0])).all() and np.isposinf(_np(got["quantile"])).all()


def test_a_row_never_decreases_along_ascending_horizons(gpu):
    c = _case(70)
    n, bt, bh = 257, c["bt"], c["bh"]
    tau = np.sort(np.concatenate([bt[::37], np.random.default_rng(2).uniform(0.0, bt[-1] + 1.0, 40), [0.0]]))
    got = _np(gpu.cox_survival_times_device(_dev(c["X"][:n]), c["cols"], c["B"], bt, bh, tau=tau)["rmst"])
    assert (np.diff(got, axis=1) >= 0).all() and (got[:, 0] == 0.0).all() and (got[:, -1] > 0).all()
    coxrmstref.check_rmst(got, _rmst_ref(gpu, c, bt, bh, tau, slice(0, n)), "ascending horizons")


def test_the_terms_are_those_of_the_curve_kernel(gpu):
    """cox_survival_device at the segment hazards gives V (n x K); any additions-only sum of the N products wd_k V_ik,
    fused or not, lies within (gamma_N + u)(1 + u) sum wd_k V_ik of the exact sum."""
    c = _case(3)
    n, bt, bh, tau = 257, c["bt"], c["bh"], c["tau"]
    t = _dev(c["X"][:n])
    hs, wd, cut = gpu.rmst_segments(bt, bh, tau)
    V = _np(gpu.cox_survival_device(t, c["cols"], c["B"], np.arange(float(hs.size)), hs)).astype(LD)
    got = _np(gpu.cox_survival_times_device(t, c["cols"], c["B"], bt, bh, tau=tau)["rmst"]).astype(LD)
    sums = np.cumsum(V * wd.astype(LD)[None, :], axis=1)
    for j, N in enumerate(cut):
        exact = sums[:, N - 1]
        bound = (coxrmstref.gamma(int(N)) + U) * (LD(1) + U) * exact
        err = np.abs(got[:, j] - exact)
        print("terms, N = %d: largest err / bound %.3f" % (N, float((err / bound).max())))
        assert (err <= bound).all(), (j, N)


def test_a_row_has_the_same_bits_alone_in_a_repeat_and_at_another_position(gpu):
    c = _case(3)
    bt, bh, tau = c["bt"], c["bh"], c["tau"]
    t = _dev(c["X"][:NMAX])
    args = (c["cols"], c["B"], bt, bh)
    got = gpu.cox_survival_times_device(t, *args, tau=tau, q=QS)
    again = gpu.cox_survival_times_device(t, *args, tau=tau, q=QS)
    for k in ("rmst", "quantile"):
        assert np.array_equal(_bits(again[k]), _bits(got[k])), k
    for i in (0, 255, 256, 511, 512, 1024):
        alone = gpu.cox_survival_times_device(t[i:i + 1], *args, tau=tau, q=QS)  # an n = 1 view of the same memory
        for k in ("rmst", "quantile"):
            assert np.array_equal(_bits(alone[k]), _bits(got[k][i:i + 1])), (i, k)
    perm = np.random.default_rng(4).permutation(NMAX)
    moved = gpu.cox_survival_times_device(_dev(c["X"][:NMAX][perm]), *args, tau=tau, q=QS)
    for k in ("rmst", "quantile"):
        assert np.array_equal(_bits(moved[k]), _bits(got[k])[perm]), k
    # the dtype of X: a float32 X and the float64 X that holds its widened values, row-major and column-major
    x32 = c["X"][:NMAX].astype(np.float32)
    for order in ("row-major", "column-major"):
        a, b = _dev(x32), _dev(x32.astype(np.float64))
        if order == "column-major":
            a, b = _dev(np.ascontiguousarray(x32.T)).T, _dev(np.ascontiguousarray(x32.astype(np.float64).T)).T
        narrow = gpu.cox_survival_times_device(a, *args, tau=tau, q=QS)
        wide = gpu.cox_survival_times_device(b, *args, tau=tau, q=QS)
        for k in ("rmst", "quantile"):
            assert np.array_equal(_bits(narrow[k]), _bits(wide[k])), (order, k)


# ----------------------------------------------------------------------------------------------------------------
# extremes
# ----------------------------------------------------------------------------------------------------------------
def test_clamped_predictors_subnormal_terms_and_nan_rows(gpu):
    c = _case(3)
    n, cols, B, bt, bh, tau = 513, c["cols"], c["B"], c["bt"], c["bh"], c["tau"]
    X = c["X"][:n].copy()
    X[::5] *= 40.0  # eta beyond +-30 in many rows: clamped
    eta, delta = evalref.eta_reference(X, cols, np.asarray(B).reshape(-1, 1), [0.0])
    big = {"eta": eta[:, 0], "delta": delta[:, 0]}
    assert (np.abs(np.asarray(eta[:, 0], dtype=np.float64)) > 30.0).sum() >= 20
    got = gpu.cox_survival_times_device(_dev(X), cols, B, bt, bh, tau=tau, q=QS)
    coxrmstref.check_rmst(_np(got["rmst"]), _rmst_ref(gpu, big, bt, bh, tau), "clamped rows")
    coxrmstref.check_quantiles(_np(got["quantile"]), coxrmstref.quantile_reference(big["eta"], big["delta"], bh,
                                                                                  gpu.survival_levels(QS)), bt, "clamped")
    # terms in and below the subnormal range: z of 700 to 750 in the later segments
    st, sh = np.arange(1.0, 65.0), np.linspace(1.0, 2000.0, 64)
    stau = np.array([3.0, 40.5, 64.0, 70.0])
    hs, wd, cut = gpu.rmst_segments(st, sh, stau)
    terms = coxsurvref.curve_reference(c["eta"][:n], c["delta"][:n], hs, "survival")["value"]
    assert ((terms < LD(2.0) ** -1022) & (terms > 0)).sum() >= 50
    got_s = _np(gpu.cox_survival_times_device(_dev(c["X"][:n]), cols, B, st, sh, tau=stau)["rmst"])
    coxrmstref.check_rmst(got_s, _rmst_ref(gpu, c, st, sh, stau, slice(0, n), adversarial=True), "subnormal terms",
                          ordinary=False)
    assert (np.diff(got_s, axis=1) >= 0).all()
    # a NaN in one support column of one row; NaN in every column outside the support
    clean = gpu.cox_survival_times_device(_dev(c["X"][:n]), cols, B, bt, bh, tau=np.append(tau, 0.0), q=QS)
    bad = c["X"][:n].copy()
    bad[321, cols[2]] = np.nan
    bad[:, np.setdiff1d(np.arange(P), cols)] = np.nan
    got = gpu.cox_survival_times_device(_dev(bad), cols, B, bt, bh, tau=np.append(tau, 0.0), q=QS)
    keep = np.arange(n) != 321
    for k in ("rmst", "quantile"):
        g = _np(got[k])
        assert np.isnan(g[321]).all() and not np.isnan(g[keep]).any(), k
        assert np.array_equal(_bits(g[keep]), _bits(_np(clean[k])[keep])), k


# ----------------------------------------------------------------------------------------------------------------
# quantiles
# ----------------------------------------------------------------------------------------------------------------
def test_quantiles_at_an_exact_level_and_above_the_last_hazard(gpu):
    n, J = 257, 8
    X = np.random.default_rng(6).standard_normal((n, 4))
    cols, B = np.array([], dtype=np.int32), np.array([])  # m = 0: e = 1
    ut, hz = np.arange(10.0, 10.0 + J), (np.arange(J) + 1.0) / 8.0
    levels = [3.0 / 8.0, np.nextafter(3.0 / 8.0, 1.0), 1.0, np.nextafter(1.0, 2.0), 1e-300, 50.0]
    got = _np(gpu.cox_survival_times_device(_dev(X), cols, B, ut, hz, hazard_levels=levels)["quantile"])
    assert (got == np.array([ut[2], ut[3], ut[7], np.inf, ut[0], np.inf])).all()
    for Jt in (1, 2, 3):  # the shortest searches
        got = _np(gpu.cox_survival_times_device(_dev(X), cols, B, ut[:Jt], hz[:Jt], hazard_levels=[0.125, 0.2, 0.375, 9.0])
                  ["quantile"])
        want = [ut[0], ut[1] if Jt > 1 else np.inf, ut[2] if Jt > 2 else np.inf, np.inf]
        assert (got == np.array(want)).all(), Jt
    flat = np.array([0.0, 0.0, 0.5, 0.5, 0.5, 2.0])  # repeated hazards: the FIRST time that reaches the level
    got = _np(gpu.cox_survival_times_device(_dev(X), cols, B, np.arange(6.0), flat, hazard_levels=[0.5, 0.25, 2.0])["quantile"])
    assert (got == np.array([2.0, 2.0, 5.0])).all()


# ----------------------------------------------------------------------------------------------------------------
# outputs, the C entry, the estimator, the bench
# ----------------------------------------------------------------------------------------------------------------
def _out(variant, n, T):
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")
    if variant == "row-major":
        b = f(n, T)
        return b, b
    if variant == "column-major":
        b = f(T, n)
        return b, b.T
    b = f(2 * n, 3 * T)  # both strides > 1
    return b, b[::2, 1::3]


def test_outputs_of_every_layout_their_errors_and_the_ledger(gpu):
    c = _case(3)
    n, cols, B, bt, bh, tau = 513, c["cols"], c["B"], c["bt"], c["bh"], c["tau"]
    t = _dev(c["X"][:n])

    class Plain:  # a device array that is not a torch tensor: the results are host arrays
        __cuda_array_interface__ = t.__cuda_array_interface__

    before = gpu.process_counters()
    want = gpu.cox_survival_times_device(t, cols, B, bt, bh, tau=tau, q=QS)
    host = gpu.cox_survival_times_device(Plain(), cols, B, bt, bh, tau=tau, q=QS)
    for k in ("rmst", "quantile"):
        assert isinstance(host[k], np.ndarray) and np.array_equal(_bits(host[k]), _bits(want[k])), k
    for vr in ("row-major", "column-major", "strided"):
        for vq in ("row-major", "column-major", "strided"):
            br, r = _out(vr, n, 4)
            bq, q = _out(vq, n, 5)
            got = gpu.cox_survival_times_device(t, cols, B, bt, bh, tau=tau, q=QS, out_rmst=r, out_quantile=q)
            assert got["rmst"] is r and got["quantile"] is q
            assert np.array_equal(_bits(r), _bits(want["rmst"])) and np.array_equal(_bits(q), _bits(want["quantile"]))
            r.fill_(-7.0)
            q.fill_(-7.0)  # the bytes outside the views are untouched
            assert bool((br == -7.0).all()) and bool((bq == -7.0).all()), (vr, vq)
    _, r = _out("row-major", n, 4)
    mixed = gpu.cox_survival_times_device(Plain(), cols, B, bt, bh, tau=tau, q=QS, out_rmst=r)  # device and host
    assert mixed["rmst"] is r and np.array_equal(_bits(r), _bits(want["rmst"]))
    assert isinstance(mixed["quantile"], np.ndarray) and np.array_equal(_bits(mixed["quantile"]), _bits(want["quantile"]))
    for name, T in (("out_rmst", 4), ("out_quantile", 5)):
        for bad, msg in ((torch.zeros((n, T + 1), dtype=torch.float64, device="cuda"), "must have shape"),
                         (torch.zeros((n, T), dtype=torch.float32, device="cuda"), "float64"),
                         (np.zeros((n, T)), "must be a device array")):
            with pytest.raises(ValueError, match=msg):
                gpu.cox_survival_times_device(t, cols, B, bt, bh, tau=tau, q=QS, **{name: bad})
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
    assert after["allocation_requests"] > before["allocation_requests"]


def test_c_abi_pointer_checks_host_strides_and_bench(gpu):
    c = _case(3)
    n, cols, B = 64, c["cols"], np.ascontiguousarray(c["B"])
    t = _dev(c["X"][:n])
    hs, wd, cut = gpu.rmst_segments(c["bt"][:40], c["bh"][:40], [0.0, c["bt"][20], 9.0])
    hz, ut, lev = np.ascontiguousarray(c["bh"][:40]), np.ascontiguousarray(c["bt"][:40]), np.array([0.01, 5.0])
    lib = gpu.lib()
    before = gpu.process_counters()

    def call(rm, qu, on_device, rs=(3, 1), qs=(2, 1)):
        a = gpu.CoxSurvtimeInput()
        a.x, a.x_dtype, a.x_row_stride, a.x_col_stride, a.n, a.p = t.data_ptr(), 0, P, 1, n, P
        a.cols, a.m, a.B = gpu._ip(cols), 3, gpu._dp(B)
        a.hs, a.wd, a.K, a.cut, a.T = gpu._dp(hs), gpu._dp(wd), hs.size, gpu._ip(cut), 3
        a.hz, a.ut, a.J, a.c, a.Q = gpu._dp(hz), gpu._dp(ut), 40, gpu._dp(lev), 2
        a.rmst_row_stride, a.rmst_col_stride, a.quant_row_stride, a.quant_col_stride = rs + qs
        a.out_on_device = on_device
        return lib.bessx_cox_survtime_device(ctypes.byref(a), rm, qu)

    want = gpu.cox_survival_times_device(t, cols, B, c["bt"][:40], c["bh"][:40], tau=[0.0, c["bt"][20], 9.0],
                                         hazard_levels=lev)
    hr, hq = np.full((n, 3), -7.0), np.full((n, 2), -7.0)
    assert call(hr.ctypes.data, hq.ctypes.data, 1) == 1 and b"rmst" in lib.bessx_last_error()  # host pointers
    dr = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    assert call(dr.data_ptr(), hq.ctypes.data, 1) == 1 and b"quant" in lib.bessx_last_error()
    small = torch.zeros(32, dtype=torch.float64, device="cuda")
    assert call(small.data_ptr(), dr.data_ptr(), 1, rs=(1 << 24, 1)) == 1  # a view that reaches past its allocation
    assert (hr == -7.0).all() and (hq == -7.0).all()
    assert call(hr.ctypes.data, hq.ctypes.data, 0) == 0, gpu.last_error()
    assert np.array_equal(_bits(hr), _bits(want["rmst"])) and np.array_equal(_bits(hq), _bits(want["quantile"]))
    sr, sq = np.full((n, 7), -7.0), np.full((5, n), -7.0)  # host results at strides of their own
    assert call(sr.ctypes.data, sq.ctypes.data, 0, rs=(7, 2), qs=(1, 2 * n)) == 0, gpu.last_error()
    assert np.array_equal(_bits(sr[:, 0:6:2]), _bits(hr)) and (sr[:, 1::2] == -7.0).all() and (sr[:, 6] == -7.0).all()
    assert np.array_equal(_bits(sq[0:4:2].T), _bits(hq)) and (sq[1::2] == -7.0).all()
    after = gpu.process_counters()
    assert after["live_device_bytes"] == before["live_device_bytes"]
    assert after["live_pinned_bytes"] == before["live_pinned_bytes"]
    for K, T in ((1000, 7), (300, 1)):
        ms = gpu.op_cox_rmst_bench(t, cols, K=K, T=T, J=100, Q=3, repeats=2)
        assert len(ms) == 4 and all(v > 0 for v in ms)


def test_the_estimator_against_the_capi_route_and_the_numpy_route(gpu):
    X, obs, status, _, _ = synth.make_cox(300, 20, 3, seed=76)
    y = np.column_stack([obs, status])
    Xd = _dev(X)
    est = linear.PdasCox(sequence=[1, 2, 3, 4])
    est.fit(Xd, y)
    with pytest.raises(ValueError, match="fit_baseline"):
        est.predict_rmst(Xd, [1.0])
    with pytest.raises(ValueError, match="fit_baseline"):
        est.predict_quantile(Xd)
    est.fit_baseline(Xd, y)
    cols = np.nonzero(est.beta)[0]
    bt, bh = est.baseline_times_, est.baseline_cumhaz_
    tau = np.array([np.median(obs), 0.0, obs.max() + 1.0, bt[3]])
    got = est.predict_rmst(Xd, tau)
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (300, 4)
    direct = gpu.cox_survival_times_device(Xd, cols, est.beta[cols], bt, bh, tau=tau, q=QS)
    assert np.array_equal(_bits(got), _bits(direct["rmst"]))
    qt = est.predict_quantile(Xd, QS)
    assert isinstance(qt, torch.Tensor) and np.array_equal(_bits(qt), _bits(direct["quantile"]))
    assert np.array_equal(_bits(est.predict_quantile(Xd)), _bits(qt[:, 2])) and tuple(est.predict_quantile(Xd).shape) == (300,)
    one = est.predict_rmst(Xd, float(tau[0]))  # (a single number: (n,), the bits of the one-horizon call)
    assert tuple(one.shape) == (300,) and np.array_equal(_bits(one), _bits(est.predict_rmst(Xd, tau[:1])[:, 0]))
    eta, delta = evalref.eta_reference(X, cols, est.beta[cols].reshape(-1, 1), [0.0])
    hs, wd, cut = gpu.rmst_segments(bt, bh, tau)
    ref = coxrmstref.rmst_reference(eta[:, 0], delta[:, 0], hs, wd, cut)
    coxrmstref.check_rmst(_np(got), ref, "estimator, device")
    host = linear.PdasCox()
    host.p, host.beta, host.coef0 = est.p, est.beta, est.coef0
    host.baseline_times_, host.baseline_cumhaz_ = bt, bh
    other = host.predict_rmst(X, tau)
    coxrmstref.check_rmst(other, ref, "estimator, numpy")
    assert (np.abs(_np(got).astype(LD) - other.astype(LD)) <= 2 * ref["bound"]).all()
    qref = coxrmstref.quantile_reference(eta[:, 0], delta[:, 0], bh, gpu.survival_levels(QS))
    coxrmstref.check_quantiles(_np(qt), qref, bt, "estimator, device")
    coxrmstref.check_quantiles(host.predict_quantile(X, QS), qref, bt, "estimator, numpy")
    with pytest.raises(ValueError, match=r"X\.shape\[1\] should be 20"):
        est.predict_rmst(Xd[:, :19], tau)
