"""Extended-precision reference and error bound for the restricted mean and quantile survival times of
bessx_cox_survtime_device, capi.cox_survival_times_device and bess_base.predict_rmst / predict_quantile (shared by
tests/test_cox_rmst_api.py and tests/test_cox_rmst_gpu.py, in the manner of tests/coxsurvref.py, whose curve_reference
supplies the term).

Definitions.  e*_i = exp(clamp(eta*_i, -30, 30)) as in coxsurvref.  RMST: with the segments (hs, wd, cut) of
capi.rmst_segments -- given data, so hg_bound = 0 -- s*_ik = exp(-(hs_k e*_i)) and out*(i, j) = sum_{k < cut_j} wd_k s*_ik.
Quantiles: z*_ig = hz_g e*_i, g*(i, j) = min{g : z*_ig >= c_j}, the result ut[g*] or +inf.  NumPy in np.longdouble; the
reference's own error is 2^-11 of every figure below and is not added.

The RMST bound is derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).  curve_reference gives b_ik with
|s_hat_ik - s*_ik| <= b_ik for the computed term (the product, the exp of 1 ulp, and TINY = 2^-1074 where the term is
subnormal).  The implementations form p_k = wd_k s_hat_k and add the N = cut_j NON-NEGATIVE products, ADDITIONS ONLY,
every one entering exactly once (the device: fma(wd_k, s_hat_k, acc) inside a piece, then the pieces in ascending
order; NumPy: a matrix-vector product per block and a running sum over the blocks).  With a separate multiplication the
product carries one rounding, |p_hat - wd s_hat| <= u wd s_hat, and N - 1 additions in any order give gamma_{N-1}
relative to the sum of the p_hat (Higham, section 4.2); with the fused form the product is exact and a term passes
through at most N roundings.  Either way, with s_hat <= s* + b,

    |out - out*| <= (1 + u) sum wd_k b_k  +  u sum wd_k s*_k  +  gamma_N (1 + u) sum wd_k (s*_k + b_k)

the sums over k < cut_j.  (A product wd_k s_hat_k below 2^-1022 adds TINY / 2: wd_k TINY of the b_k that curve_reference
gives there covers it for wd_k >= 1/2, and no ordinary case has such a term; the adversarial cases add N TINY.)
cut_j = 0 gives exactly 0.0 and a bound of 0.  So that a loose bound cannot hide a failure, check_rmst also asserts,
unless told that the case is adversarial, that the bound is at most 1e-9 relative (for 4099 rows, |eta| <= 5 and about
2500 segments the derivation gives at most 3.5e-13).

Quantiles are checked by index.  The computed product is z_hat = fl(hz_g e_hat_i) with e_hat = e* (1 + r), |r| <= rho_i
(coxevalref), so |z_hat - z*| <= z* (rho_i + u), and the comparison z_hat >= c can differ from z* >= c only where
|z* - c| <= dz = z* (rho_i + u) + u c.  A (row, level) pair is EXCUSED from the index check only when that holds at
g* - 1 or at g*; check_quantiles asserts that at most 1 % of the pairs are.

self_check() holds rmst_reference (through capi.rmst_segments) to an independent statement -- the integral of the step
function taken interval by interval of the baseline's own times, row by row, with no segment list -- and
quantile_reference to a linear scan, at n <= 50."""
import numpy as np

import coxsurvref
import evalref

LD = np.longdouble
U = evalref.U
gamma = evalref.gamma
BOUND_CAP = 1e-9
TINY = coxsurvref.TINY


def rmst_reference(eta, delta, hs, wd, cut, adversarial=False):
    """eta, delta (n,) in row order from evalref.eta_reference (c = 0); hs, wd (K,), cut (T,) from capi.rmst_segments.
    Returns {"value": (n, T), "bound": (n, T)} in longdouble."""
    hs, wd = np.asarray(hs, dtype=np.float64).reshape(-1), np.asarray(wd).astype(LD).reshape(-1)
    cut = np.asarray(cut).reshape(-1).astype(np.int64)
    n, T, K = np.asarray(eta).reshape(-1).size, cut.size, int(cut.max()) if cut.size else 0
    value, bound = np.zeros((n, T), dtype=LD), np.zeros((n, T), dtype=LD)
    if K == 0:
        return {"value": value, "bound": bound}
    cur = coxsurvref.curve_reference(eta, delta, hs[:K], "survival")
    S = np.cumsum(cur["value"] * wd[None, :K], axis=1)  # sum wd s*
    A = np.cumsum(cur["bound"] * wd[None, :K], axis=1)  # sum wd b
    for j in range(T):
        N = int(cut[j])
        if N == 0:
            continue
        s, a = S[:, N - 1], A[:, N - 1]
        value[:, j] = s
        bound[:, j] = (LD(1) + U) * a + U * s + gamma(N) * (LD(1) + U) * (s + a) + (LD(N) * TINY if adversarial else LD(0))
    return {"value": value, "bound": bound}


def check_rmst(got, ref, what="", ordinary=True, rows=None):
    """Print the figures, then assert the bound for every element (of the rows given, default all) and (ordinary cases)
    that the bound itself is at most 1e-9 relative."""
    got = np.asarray(got).astype(LD)
    assert got.shape == ref["value"].shape, (what, got.shape, ref["value"].shape)
    val, bnd = ref["value"], ref["bound"]
    if rows is not None:
        got, val, bnd = got[rows], val[rows], bnd[rows]
    err = np.abs(got - val)
    rel = bnd / np.where(val > 0, val, LD(1))
    worst = np.unravel_index(int(np.argmax(err / np.where(bnd > 0, bnd, LD(1)))), err.shape)
    print("%s: rmst, at the worst element err %.3e against bound %.3e (value %.6e); largest relative bound %.3e" % (
        what, float(err[worst]), float(bnd[worst]), float(val[worst]), float(rel.max())))
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert (err <= bnd).all(), (what, worst, float(err[worst]), float(bnd[worst]))
    if ordinary:
        assert float(rel.max()) <= BOUND_CAP, (what, "the bound is too loose for an ordinary case", float(rel.max()))


def quantile_reference(eta, delta, hz, c):
    """eta, delta (n,); hz (J,) non-decreasing; c (Q,) > 0.  Returns {"index": (n, Q) int64, J where no g qualifies,
    "excused": (n, Q) bool, "gap": (n, Q) the smallest |z* - c| / c over g* - 1 and g*}."""
    eta, delta = np.asarray(eta, dtype=LD).reshape(-1), np.asarray(delta, dtype=LD).reshape(-1)
    hz, c = np.asarray(hz).astype(LD).reshape(-1), np.asarray(c).astype(LD).reshape(-1)
    n, J, Q = eta.size, hz.size, c.size
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    rho = coxsurvref._rho(delta) + U
    index = np.full((n, Q), J, dtype=np.int64)
    excused = np.zeros((n, Q), dtype=bool)
    gap = np.full((n, Q), np.inf)
    if J == 0:
        return {"index": index, "excused": excused, "gap": gap}
    z = e[:, None] * hz[None, :]
    r = np.arange(n)
    for j in range(Q):
        hit = z >= c[j]
        g = np.where(hit.any(axis=1), hit.argmax(axis=1), J)
        index[:, j] = g
        for at in (g - 1, g):
            ok = (at >= 0) & (at < J)
            za = z[r, np.clip(at, 0, J - 1)]
            d = np.abs(za - c[j])
            excused[:, j] |= ok & (d <= za * rho + U * c[j])
            gap[:, j] = np.where(ok, np.minimum(gap[:, j], np.asarray(d / c[j], dtype=np.float64)), gap[:, j])
    return {"index": index, "excused": excused, "gap": gap}


def check_quantiles(got, ref, ut, what="", max_excused=0.01):
    """got (n, Q) times; ut (J,) strictly ascending.  Every result is a base time or +inf, its index is the reference's
    unless the pair is excused, and at most max_excused of the pairs are excused."""
    got, ut = np.asarray(got, dtype=np.float64), np.asarray(ut, dtype=np.float64).reshape(-1)
    J = ut.size
    assert got.shape == ref["index"].shape, (what, got.shape, ref["index"].shape)
    assert not np.isnan(got).any(), what
    idx = np.where(np.isinf(got), J, np.searchsorted(ut, np.where(np.isinf(got), 0.0, got)))
    assert ((idx == J) | (ut[np.minimum(idx, max(J - 1, 0))] == got)).all() if J else (idx == 0).all(), what
    share = float(ref["excused"].mean())
    wrong = (idx != ref["index"]) & ~ref["excused"]
    print("%s: quantiles, %d pairs, %d excused (%.3f %%), %d reach no time, smallest relative gap %.3e, %d off" % (
        what, idx.size, int(ref["excused"].sum()), 100.0 * share, int((ref["index"] == J).sum()),
        float(ref["gap"].min()) if idx.size else np.inf, int(wrong.sum())))
    assert not wrong.any(), (what, np.argwhere(wrong)[:5])
    assert (np.abs(idx - ref["index"]) <= 1).all(), what  # (an excused pair moves by one step at most)
    assert share <= max_excused, (what, share)


def brute_force_rmst(eta, base_times, base_cumhaz, tau):
    """RMST by the definition, row by row and horizon by horizon, longdouble: the integral of the step function taken
    over the intervals between consecutive baseline times, each clipped to [0, tau]; widths formed in fp64 as the
    implementation's are."""
    eta = np.asarray(eta, dtype=LD).reshape(-1)
    e = np.exp(np.clip(eta, LD(-30), LD(30)))
    bt, bh = np.asarray(base_times, dtype=np.float64), np.asarray(base_cumhaz, dtype=np.float64)
    knots = np.concatenate([[0.0], bt, [np.inf]])
    haz = np.concatenate([[0.0], bh])  # on [knots[g], knots[g + 1])
    taus = np.unique(np.asarray(tau, dtype=np.float64))
    out = np.zeros((eta.size, len(tau)), dtype=LD)
    for j, tj in enumerate(tau):
        for i in range(eta.size):
            total = LD(0)
            for g in range(haz.size):
                lo, hi = knots[g], min(knots[g + 1], tj)
                if hi <= lo:
                    continue
                # the implementation's widths: between consecutive breakpoints, the other horizons among them
                cuts = np.concatenate([[lo], taus[(taus > lo) & (taus < hi)], [hi]])
                width = np.sum((cuts[1:] - cuts[:-1]).astype(LD))
                total += width * np.exp(-(LD(haz[g]) * e[i]))
            out[i, j] = total
    return out


def self_check(seed=0):
    from bess_amd import capi
    rng = np.random.default_rng(seed)
    for n, J in ((1, 0), (2, 1), (13, 7), (50, 40)):
        eta = rng.normal(0.0, 1.5, n).astype(LD)
        bt = np.cumsum(rng.uniform(0.05, 0.4, J))
        bh = np.cumsum(rng.uniform(0.0, 0.3, J))
        tau = np.array([0.0, 0.01, 1.0, 1.0, 100.0] + ([bt[J // 2], bt[-1]] if J else []))
        tau = tau[rng.permutation(tau.size)]
        hs, wd, cut = capi.rmst_segments(bt, bh, tau)
        ref = rmst_reference(eta, np.zeros(n, dtype=LD), hs, wd, cut)
        want = brute_force_rmst(eta, bt, bh, tau)
        tol = LD(hs.size + 2) * LD(2.0) ** -61 * np.maximum(want, LD(1e-300))
        assert (np.abs(ref["value"] - want) <= tol).all(), (n, J, ref["value"], want)
        c = np.array([0.05, 0.7, 3.0])
        qr = quantile_reference(eta, np.zeros(n, dtype=LD), bh, c)
        e = np.exp(np.clip(eta, LD(-30), LD(30)))
        for i in range(n):
            for j in range(c.size):
                g = next((g for g in range(J) if LD(bh[g]) * e[i] >= LD(c[j])), J)
                assert qr["index"][i, j] == g, (n, J, i, j)
    return True
