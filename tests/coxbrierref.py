"""Extended-precision reference and error bound for the IPCW Brier score of bessx_cox_brier_device,
capi.cox_brier_device / ipcw_weights / censoring_km and bess_base.brier_survival (shared by tests/test_cox_brier_api.py
and tests/test_cox_brier_gpu.py, in the manner of tests/coxsurvref.py, whose allowance for exp and whose treatment of
gradual underflow are used as they stand).

Definitions.  eta*(i, r) = sum_k x(i, cols[k]) B[k, r], e* = exp(clamp(eta*, -30, 30)), z*(i, j, r) = hg(j, r) e*(i, r),
S* = exp(-z*), q* = -expm1(-z*); term* = a_i S*^2 where time_i <= t_j (inclusive), b_j q*^2 otherwise;
BS*(j, r) = sum_i w_i term* / W*, W* = sum_i w_i.  hg, times, time, w, a and b are DATA here: the fp64 values the
implementation was given (a and b are checked on their own, below).  NumPy in np.longdouble; the reference's own error is
2^-11 of every figure below and is not added.

The bound is derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u), TINY = 2^-1074.  Each floating-point
operation of the implementations is counted once (a fused multiply-add only removes one); the device kernel
(bessx_k_coxbrier.hip) and the NumPy route of bess_base._brier_host have the same form.

    e_hat  = e* (1 + r), |r| <= rho_i = expm1(Delta_i) (1 + 2 u) + 2 u        (Delta of evalref.eta_reference; coxevalref)
    z_hat  = hg * e_hat                 one multiplication: |z_hat - z*| <= dz = z* (rho_i + u) + TINY / 2    (0 where z* = 0)
    S_hat  = exp(-z_hat)                1 ulp = 2 u relative, TINY below 2^-1022 (coxsurvref):
                                        |S_hat - S*| <= dS = S* expm1(dz) + max(2 u S* (1 + expm1(dz)), TINY)
    q_hat  = -expm1(-z_hat)             expm1(-z_hat) - expm1(-z*) = S* expm1(z* - z_hat), and the function's own error is
                                        an ALLOWANCE of 2 ulp = 4 u relative: the ROCm documentation installed with the
                                        compiler states no figure for expm1, so this one is ASSUMED -- nobody measured it
                                        (glibc's, which NumPy calls, is below 1 ulp):
                                        |q_hat - q*| <= dq = S* expm1(dz) + 4 u (q* + S* expm1(dz)) + TINY
                                        z* = 0 gives S_hat = 1 and q_hat = 0 exactly: dS = dq = 0 there.
    v_hat  = S_hat^2 or q_hat^2         one multiplication: |v_hat - v*| <= dv = 2 y* dy + dy^2 + u (y* + dy)^2 + TINY
    the two weights                     w_i a_i (one rounding) times v (one), or w_i v (one) and, once per sum, b_j times the
                                        sum (one): two roundings either way,
                                        |term_hat - term*| <= dterm = c* (dv + gamma_2 (v* + dv)),  c* = w a or w b
    the sum                             n non-negative terms, additions only, every term entering once: gamma_D relative to
                                        the sum of the computed terms, D the longest chain of additions.  Device: a thread
                                        adds ceil(rows of a slab / G) terms, G = row groups (a function of T), then G - 1
                                        group sums, A + b Q, then the slabs: D = ceil(min(n, 1024) / G) + G + slabs
                                        (device_depth).  Host: any order, D = n.
    W_hat, the division                 W_hat = W* (1 + gamma_{n-1}) (a sum of non-negative weights in any order), one
                                        division: relative gamma_{n+1} on top.

    |BS_hat - BS*| <= (sum_i dterm_i + gamma_D sum_i (w term*_i + dterm_i)) / W* + gamma_{n+1} BS* (1 + 1e-9)

Every term is non-negative, so the bound is relative to BS*.  So that it cannot grow until it hides a failure,
brier_reference asserts for every input that bound <= inforef.REL_CEILING (1e-9) x BS* + 2^-1000 (the absolute part covers
only what gradual underflow forces: squares of survivals below 2^-511).

IPCW weights.  ipcw_reference is the explicit product definition in longdouble: d_u = sum w [time = u, status = 0],
Y_u = sum w [time > u] + d_u, G(t) = prod_{u <= t} (1 - d_u / Y_u), a_i = status_i / G(time_i-) (0 where w_i = 0 or
status_i = 0), b_j = 1 / G(t_j).  capi forms each factor as (Y_u - d_u) / Y_u from two sums of non-negative weights
(gamma_n each), one addition and one division, multiplies K factors (K: the censoring times up to t) and divides once:
relative error at most K (2 gamma_n + 3 u) + 2 u, which ipcw_bound returns.

self_check() holds the reference to a brute-force double loop over (i, j) and to the three identities listed there."""
import numpy as np

import coxsurvref
import evalref
import inforef

LD = np.longdouble
U = evalref.U
gamma = evalref.gamma
TINY = coxsurvref.TINY
REL_CEILING = inforef.REL_CEILING
ABS_FLOOR = LD(2.0) ** -1000
EXPM1_ALLOW = LD(4) * U  # 2 ulp, ASSUMED (see above)
SLAB_ROWS, THREADS = 1024, 256  # CXB_ROWS, CXB_T of bessx_k_coxbrier.hip


def row_groups(T):
    lg = 0
    while lg < 8 and (1 << lg) < T:
        lg += 1
    return THREADS >> lg


def device_depth(n, T):
    G = row_groups(T)
    return -(-min(n, SLAB_ROWS) // G) + G + -(-n // SLAB_ROWS)


def _ld(a):
    return np.asarray(a).astype(LD)


def brier_reference(eta, delta, hg, times, time, w, a, b, depth, what=""):
    """eta, delta (n, R) from evalref.eta_reference (c = 0); hg (T, R); times, b (T,); time, a (n,); w (n,) or None;
    depth: D.  Returns {"value", "bound"}: (T, R) longdouble, after the ceiling assertion."""
    eta, delta, hg = _ld(eta), _ld(delta), _ld(hg)
    n, R = eta.shape
    T = hg.shape[0]
    times, time = np.asarray(times, dtype=np.float64).reshape(-1), np.asarray(time, dtype=np.float64).reshape(-1)
    w = np.ones(n, dtype=LD) if w is None else _ld(w).reshape(-1)
    a, b = _ld(a).reshape(-1), _ld(b).reshape(-1)
    assert hg.shape == (T, R) and times.size == T and b.size == T and time.size == n and a.size == n
    W = w.sum()
    left = time[:, None] <= times[None, :]
    c = np.where(left, (w * a)[:, None], w[:, None] * b[None, :])
    value, bound = np.zeros((T, R), dtype=LD), np.zeros((T, R), dtype=LD)
    one = LD(1)
    for r in range(R):
        e = np.exp(np.clip(eta[:, r], LD(-30), LD(30)))
        rho = coxsurvref._rho(delta[:, r])
        z = e[:, None] * hg[None, :, r]
        pos = z > 0
        dz = np.where(pos, z * (rho + U)[:, None] + TINY / LD(2), LD(0))
        grow = np.expm1(dz)
        S = np.exp(-z)
        q = -np.expm1(-z)
        dS = np.where(pos, S * grow + np.maximum(LD(2) * U * S * (one + grow), TINY), LD(0))
        dq = np.where(pos, S * grow + EXPM1_ALLOW * (q + S * grow) + TINY, LD(0))
        y, dy = np.where(left, S, q), np.where(left, dS, dq)
        v = y * y
        dv = np.where(pos, LD(2) * y * dy + dy * dy + U * (y + dy) ** 2 + TINY, LD(0))
        term = c * v
        dterm = c * (dv + gamma(2) * (v + dv))
        bs = term.sum(axis=0) / W
        value[:, r] = bs
        bound[:, r] = (dterm.sum(axis=0) + gamma(depth) * (term + dterm).sum(axis=0)) / W + gamma(n + 1) * bs * (
            one + LD(1e-9))
    ok = bound <= REL_CEILING * value + ABS_FLOOR
    assert ok.all(), (what, "the derived bound exceeds its ceiling: choose other inputs",
                      float((bound / np.where(value > 0, value, one)).max()))
    return {"value": value, "bound": bound}


def brute_force_brier(eta, hg, times, time, w, a, b):
    """The definition stated element by element, a double loop over (i, j) per model, longdouble: (T, R)."""
    eta, hg = _ld(eta), _ld(hg)
    n, R = eta.shape
    T = hg.shape[0]
    w = np.ones(n, dtype=LD) if w is None else _ld(w).reshape(-1)
    a, b = _ld(a).reshape(-1), _ld(b).reshape(-1)
    out = np.zeros((T, R), dtype=LD)
    for r in range(R):
        for j in range(T):
            s = LD(0)
            for i in range(n):
                z = hg[j, r] * np.exp(min(max(eta[i, r], LD(-30)), LD(30)))
                if time[i] <= times[j]:
                    s += w[i] * a[i] * np.exp(-z) ** 2
                else:
                    s += w[i] * b[j] * (LD(1) - np.exp(-z)) ** 2
            out[j, r] = s / w.sum()
    return out


def check_brier(got, ref, what=""):
    """Print error against bound for every entry, then assert the bound."""
    got = _ld(got)
    assert got.shape == ref["value"].shape, (what, got.shape, ref["value"].shape)
    err = np.abs(got - ref["value"])
    for j in range(got.shape[0]):
        print("%s: t[%d] " % (what, j) + "  ".join("err %.2e / bound %.2e (BS %.6e)" % (
            float(err[j, r]), float(ref["bound"][j, r]), float(ref["value"][j, r])) for r in range(got.shape[1])))
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    worst = np.unravel_index(int(np.argmax(err - ref["bound"])), err.shape)
    assert (err <= ref["bound"]).all(), (what, worst, float(err[worst]), float(ref["bound"][worst]))


def km_reference(time, status, w):
    """(u, d_u, Y_u, factor_u) of the censoring estimate by the explicit definition, longdouble."""
    time, status = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(status, dtype=np.float64).reshape(-1)
    w = np.ones(time.size, dtype=LD) if w is None else _ld(w).reshape(-1)
    u = np.unique(time)
    d = np.array([w[(time == t) & (status == 0)].sum() for t in u], dtype=LD)
    Y = np.array([w[time > t].sum() for t in u], dtype=LD) + d
    f = np.where(d > 0, LD(1) - d / np.where(Y > 0, Y, LD(1)), LD(1))
    return u, d, Y, f


def ipcw_reference(time, status, times, w):
    """{"a": (n,), "b": (T,) longdouble (inf where G = 0), "ka", "kb": the factors behind each entry, "G": (u, G)}."""
    time, status = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(status, dtype=np.float64).reshape(-1)
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    wl = np.ones(time.size, dtype=LD) if w is None else _ld(w).reshape(-1)
    u, d, Y, f = km_reference(time, status, w)
    a, ka = np.zeros(time.size, dtype=LD), np.zeros(time.size, dtype=np.int64)
    for i in range(time.size):
        if status[i] != 0 and wl[i] > 0:
            use = u < time[i]
            a[i], ka[i] = LD(1) / np.prod(f[use]), int((use & (d > 0)).sum())
    b, kb = np.zeros(times.size, dtype=LD), np.zeros(times.size, dtype=np.int64)
    for j in range(times.size):
        use = u <= times[j]
        G = np.prod(f[use])
        b[j], kb[j] = (LD(1) / G if G > 0 else LD(np.inf)), int((use & (d > 0)).sum())
    return {"a": a, "b": b, "ka": ka, "kb": kb, "G": (u, np.cumprod(f))}


def ipcw_bound(k, n):
    """Relative error bound of an a or b behind k factors on n rows."""
    return _ld(k) * (LD(2) * gamma(n) + LD(3) * U) + LD(2) * U


def check_ipcw(row_a, time_b, ref, n, what=""):
    for name, got, val, k in (("a", row_a, ref["a"], ref["ka"]), ("b", time_b, ref["b"], ref["kb"])):
        err, bnd = np.abs(_ld(got) - val), ipcw_bound(k, n) * val
        print("%s: %s: largest err %.3e, largest bound %.3e" % (what, name, float(err.max(initial=0)),
                                                               float(bnd.max(initial=0))))
        assert (err <= bnd).all(), (what, name)
        assert ((val == 0) == (np.asarray(got) == 0)).all(), (what, name)


def null_reference(time, status, w, times, a, b):
    """BS_null (T,) in longdouble: the weighted Kaplan-Meier survival of the rows through the Brier formula."""
    time, status = np.asarray(time, dtype=np.float64).reshape(-1), np.asarray(status, dtype=np.float64).reshape(-1)
    wl = np.ones(time.size, dtype=LD) if w is None else _ld(w).reshape(-1)
    a, b = _ld(a).reshape(-1), _ld(b).reshape(-1)
    out = np.zeros(len(times), dtype=LD)
    for j, t in enumerate(np.asarray(times, dtype=np.float64).reshape(-1)):
        S = LD(1)
        for v in np.unique(time[(status != 0) & (time <= t)]):
            ev, risk = wl[(time == v) & (status != 0)].sum(), wl[time >= v].sum()
            if ev > 0:
                S *= LD(1) - ev / risk
        out[j] = (S * S * (wl * a)[time <= t].sum() + (LD(1) - S) ** 2 * b[j] * wl[time > t].sum()) / wl.sum()
    return out


def self_check(seed=0):
    """At n <= 300: (1) brier_reference against the brute-force double loop; (2) censoring=None with every status 1
    equals the mean of (1{time > t} - S)^2; (3) hg = 0 gives BS[j] = (1 / W) sum_{time_i <= t_j} w_i a_i exactly in the
    reference; (4) the IPCW identity of Kaplan-Meier weights, sum_i w_i a_i [time_i <= t] + b(t) sum_i w_i [time_i > t] = W
    for every admissible t, to a few n u."""
    rng = np.random.default_rng(seed)
    for n, weighted in ((1, False), (2, True), (37, False), (300, True)):
        R, T = 2, 7
        eta = rng.normal(0.0, 1.5, (n, R)).astype(LD)
        time = np.round(rng.exponential(1.0, n), 1) + 0.1  # (many ties)
        status = (rng.uniform(size=n) < 0.6).astype(np.float64)
        w = None
        if weighted:
            w = rng.integers(0, 9, n) / 4.0
            w[0] = 1.0
        wl = np.ones(n, dtype=LD) if w is None else _ld(w)
        times = np.sort(np.concatenate([[0.05], rng.choice(time, 3), rng.uniform(0.0, time.max() * 0.9, 3)]))
        times = times[times < time.max()]
        T = times.size
        hg = np.cumsum(rng.uniform(0.0, 0.5, (T, R)), axis=0)
        ip = ipcw_reference(time, status, times, w)
        a, b = ip["a"].astype(np.float64), ip["b"].astype(np.float64)
        zero = np.zeros((n, R), dtype=LD)
        ref = brier_reference(eta, zero, hg, times, time, w, a, b, n, "self_check")
        brute = brute_force_brier(eta, hg, times, time, w, a, b)                                           # (1)
        assert (np.abs(ref["value"] - brute) <= LD(n + 8) * LD(2.0) ** -58 * np.maximum(brute, LD(1e-300))).all(), n
        ones = np.ones(n)
        plain = brier_reference(eta, zero, hg, times, time, w, ones, np.ones(T), n, "self_check")["value"]  # (2)
        for r in range(R):
            S = np.exp(-np.exp(np.clip(eta[:, r], -30, 30))[:, None] * _ld(hg)[None, :, r])
            mse = (wl[:, None] * ((time[:, None] > times[None, :]).astype(LD) - S) ** 2).sum(axis=0) / wl.sum()
            assert (np.abs(plain[:, r] - mse) <= LD(n + 8) * LD(2.0) ** -58 * np.maximum(mse, LD(1e-300))).all(), n
        flat = brier_reference(eta, zero, np.zeros((T, R)), times, time, w, a, b, n, "self_check")["value"]  # (3)
        want = np.array([(wl * _ld(a))[time <= t].sum() for t in times], dtype=LD) / wl.sum()
        assert np.array_equal(flat[:, 0], want) and np.array_equal(flat[:, 1], want), n
        W = wl.sum()                                                                                        # (4)
        for j, t in enumerate(times):
            tot = (wl * ip["a"])[time <= t].sum() + ip["b"][j] * wl[time > t].sum()
            assert abs(tot - W) <= LD(4 * n + 8) * U * W, (n, j, float(tot), float(W))
    return True
