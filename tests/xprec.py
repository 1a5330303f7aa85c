"""Extended-precision reference for the LM hot path: pure NumPy in np.longdouble (x86: 64-bit mantissa, eps 1.08e-19),
no GPU, no oracle.  It restates the OPERATIONS of the reference (Normalize + add_weight, the
restricted least-squares fit, LmMetric's losses, get_A's sacrifice scores, Gram columns), not the kernels.

Conventions (src/normalize.cpp:20-46, src/Data.h:70-77, src/Algorithm.h:1097-1135, src/Metric.h:145-190):
  normalised design Xn: column j = sqrt(n) (x_j - mean_j) / norm_j, mean_j = w.x_j / n, norm_j = sqrt(w.(x_j - mean_j)^2),
  LM rows then times sqrt(w_i); y likewise centred and weighted;
  a row set is a 0/1 mask m over the rows (None = all rows), nt its number of rows;
  restricted fit on support A: (X_A^T diag(m) X_A + lam I) b = X_A^T (m o y);
  train_loss = |y - X_A b|^2 / n over ALL rows, test_loss = sum over the rows outside m / (2 (n - nt));
  scores: d = X^T (m o (y - X_A b)) / nt - 2 lam beta, phi_j = sqrt(2 lam + x_j.(m o x_j) / nt), bd = (phi beta + d / phi)^2.

The module also holds the seeded designs both test files use (designs()) and the assertion helpers whose bounds the
issue fixed (assert_*), so that the CPU file can show each of them failing on a perturbed input."""
import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
# x86 extended format (64-bit mantissa)?  Data, not an assertion: tests/test_xprec_reference.py asserts it where the reference
# is used on the CPU, the GPU tests skip with that reason where it does not hold.
EXTENDED = EPS_LD < 2e-19
U = 2.0 ** -53  # unit roundoff of fp64

# ---- the bounds (fixed by the issue; see the docstrings of the assert_* helpers) -----------------------------------
FIT_RESIDUAL = 1e-13  # an iterate is accepted only if |q - (G + lam I) x| <= 1e-13 |q|
FIT_MARGIN = 4.0
LOSS_RTOL = 2e-10     # DESIGN 3a promises 1e-10 for the loss identity; 2 covers the division and the direct pass
GRAM_FACTOR = 32.0
NORM_FACTOR = 4.0
SCORE_C_NUMPY = 64.0  # fp64 NumPy evaluating the two score formulas stays inside the forward-error model with this c


def ld(a):
    return np.asarray(a, dtype=LD)


def _mask(n, mask):
    return np.ones(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)


def normalize(X, y, w, data_type=1, is_normal=True, add_weight=True):
    """Data::normalize (+ add_weight) in longdouble.  Returns (Xn, yn, x_mean, x_norm, y_mean), all longdouble;
    data_type 1: X and y centred; 2: X centred; 3: neither (Normalize, Normalize3, Normalize4)."""
    X, y, w = ld(X).copy(), ld(y).copy(), ld(w)
    n, p = X.shape
    x_mean, x_norm, y_mean = np.zeros(p, dtype=LD), np.ones(p, dtype=LD), LD(0)
    if is_normal:
        if data_type in (1, 2):
            x_mean = (w @ X) / LD(n)
            X -= x_mean
        if data_type == 1:
            y_mean = (y @ w) / LD(n)
            y -= y_mean
        x_norm = np.sqrt(w @ (X * X))
        X *= np.sqrt(LD(n)) / x_norm
    if add_weight:
        sw = np.sqrt(w)
        X *= sw[:, None]
        y *= sw
    return X, y, x_mean, x_norm, y_mean


def gram_columns(Xn, mask, cols):
    """X^T diag(m) X[:, cols] in longdouble (p x len(cols))."""
    X = ld(Xn)
    m = _mask(X.shape[0], mask)
    Xm = X[m]
    return Xm.T @ np.ascontiguousarray(Xm[:, np.asarray(cols, dtype=int)])


def cond(G):
    """2-norm condition number of a symmetric positive definite matrix (fp64 eigenvalues: two digits are plenty)."""
    ev = np.linalg.eigvalsh(np.asarray(G, dtype=np.float64))
    return float(ev[-1] / ev[0])


def restricted_fit(Xn, y, mask, A, lam, rounds=3):
    """The minimiser on support A by mixed-precision iterative refinement: fp64 solves with the fp64 Gram, the residual
    X_A^T (m o (y - X_A b)) - lam b accumulated in longdouble.  Returns (b longdouble, info) with info = {"kkt": the
    solution's own relative residual |.|_2 / |q|_2, "cond": cond_2(G_A + lam I), "b64": the plain fp64 solve}."""
    A = np.asarray(A, dtype=int)
    m = _mask(np.shape(Xn)[0], mask)
    XA = ld(np.asarray(Xn)[:, A][m])
    ym = ld(y)[m]
    XA64 = XA.astype(np.float64)
    G = XA64.T @ XA64 + float(lam) * np.eye(A.size)
    q = XA.T @ ym
    b64 = np.linalg.solve(G, q.astype(np.float64))
    b = ld(b64)
    for _ in range(rounds):
        r = XA.T @ (ym - XA @ b) - LD(lam) * b
        b = b + ld(np.linalg.solve(G, r.astype(np.float64)))
    r = XA.T @ (ym - XA @ b) - LD(lam) * b
    qn = float(np.sqrt(q @ q))
    return b, {"kkt": float(np.sqrt(r @ r)) / max(qn, 1e-300), "cond": cond(G), "b64": b64, "q_norm": qn}


def loss(Xn, y, mask, A, b):
    """(train_loss, test_loss) of LmMetric for coefficients b on support A, longdouble sums of the fp64 or longdouble
    inputs: train_loss over all rows / n; test_loss over the rows outside the mask / (2 n_test), 0 without a mask."""
    A = np.asarray(A, dtype=int)
    e = ld(y) - ld(np.asarray(Xn)[:, A]) @ ld(b)
    n = e.size
    tr = (e @ e) / LD(n)
    te = LD(0)
    if mask is not None:
        t = ~_mask(n, mask)
        te = (e[t] @ e[t]) / LD(2 * max(int(t.sum()), 1))
    return tr, te


def scores(Xn, y, mask, A, b, lam, X_ld=None):
    """get_A's d, phi and bd for the model (A, b), in longdouble, plus the magnitude sums of the forward-error model
    (fp64 is enough for magnitudes):
    S_cov_j = (sum_i |x_ij y_i| + sum_a |b_a| sum_i |x_ij x_ia|) / nt + 2 lam |beta_j| for d formed from Gram columns.
    S_cov sums the magnitudes of the ELEMENTARY products: x_j.y and every G_ja are themselves length-nt fp64 dot products
    whose rounding the difference inherits.  The shorter |x_j.y| + sum_a |G_ja b_a| is no forward-error model of that
    operation: it is ~0 for a column uncorrelated with y at beta = 0, where fp64 NumPy evaluating the covariance formula
    needs c = 13582 under it (iid design, column 525; tests/test_xprec_reference.py measures c under the model used here).
    S_stream_j = S_cov_j + sum_i |x_ij r_i| / nt for d formed from the residual: r_i = y_i - sum_a x_ia b_a is formed in
    fp64 first and carries u (|y_i| + sum_a |x_ia b_a|) of rounding into the sum, which sum_i |x_ij r_i| alone leaves out
    (fp64 NumPy needs c = 76 under that shorter model at tr / yy = 1e-6, 60 at 3e-6 and growing with the signal-to-noise
    ratio).  Neither form is accurate relative to the residual: both lose what |y| / |r| says.
    X_ld: the longdouble copy of Xn if the caller keeps one."""
    A = np.asarray(A, dtype=int)
    X64 = np.asarray(Xn, dtype=np.float64)
    X = ld(Xn) if X_ld is None else X_ld
    n, p = X.shape
    m = _mask(n, mask)
    nt = LD(int(m.sum()))
    Xm, ym = X[m], ld(y)[m]
    beta = np.zeros(p, dtype=LD)
    beta[A] = ld(b)
    r = ym - Xm[:, A] @ ld(b)
    d = (Xm.T @ r) / nt - 2 * LD(lam) * beta
    phi = np.sqrt(2 * LD(lam) + np.einsum("ij,ij->j", Xm, Xm) / nt)
    t = phi * beta + d / phi
    X64m = X64[m]
    b64 = np.asarray(b, dtype=np.float64)
    ridge = 2 * float(lam) * np.abs(beta.astype(np.float64))
    aX = np.abs(X64m)
    S_cov = (aX.T @ np.abs(ym.astype(np.float64)) + aX.T @ (aX[:, A] @ np.abs(b64))) / float(nt) + ridge
    S_stream = S_cov + (aX.T @ np.abs(r.astype(np.float64))) / float(nt)
    return {"d": d, "phi": phi, "t": t, "bd": t * t, "S_cov": S_cov, "S_stream": S_stream}


def scores_fp64(Xn, y, mask, A, b, lam, form):
    """fp64 NumPy evaluating the two formulas the library uses (the CPU stand-in for the kernels): form "cov":
    d = (X^T (m o y) - sum_a g_a b_a) / nt from Gram columns; form "stream": d = X^T r / nt from the residual."""
    A = np.asarray(A, dtype=int)
    X = np.asarray(Xn, dtype=np.float64)
    m = _mask(X.shape[0], mask)
    Xm, ym = X[m], np.asarray(y, dtype=np.float64)[m]
    nt = float(m.sum())
    beta = np.zeros(X.shape[1])
    beta[A] = np.asarray(b, dtype=np.float64)
    if form == "cov":
        d = (Xm.T @ ym - (Xm.T @ Xm[:, A]) @ beta[A]) / nt - 2 * lam * beta
    else:
        d = Xm.T @ (ym - Xm[:, A] @ beta[A]) / nt - 2 * lam * beta
    phi = np.sqrt(2 * lam + (Xm * Xm).sum(axis=0) / nt)
    return (phi * beta + d * (1.0 / phi)) ** 2


def score_error_units(bd, ref, form):
    """max_j |bd_j - bd*_j| / (what the forward-error model allows with c = 1): dd_j = u S_j is the model's error of d_j,
    pushed through bd = t^2, t = phi beta + d / phi: 2 |t| dd / phi + (dd / phi)^2, plus u t^2 for the rounding of phi,
    the division and the square themselves.  Returns (largest ratio, its column)."""
    S = ref["S_cov"] if form == "cov" else ref["S_stream"]
    phi, t = ref["phi"].astype(np.float64), np.abs(ref["t"].astype(np.float64))
    e = U * S / phi
    allowed = 2 * t * e + e * e + U * t * t
    ratio = np.abs((ld(bd) - ref["bd"]).astype(np.float64)) / np.maximum(allowed, 1e-300)
    j = int(np.argmax(ratio))
    return float(ratio[j]), j


# ---- assertion helpers: one place for every bound, shared by the CPU and the GPU file -------------------------------
def assert_fit_close(b, b_ref, condG, what):
    """|b - b*|_2 <= 4 * 1e-13 * cond_2(G_A + lam I) * |b*|_2: 1e-13 is the documented acceptance residual of the solvers,
    cond turns a residual into a solution error, 4 covers the fp64 rounding of the right-hand side and the commit.
    Returns the fraction of the bound used."""
    b_ref = ld(b_ref)
    diff = ld(b) - b_ref
    err = float(np.sqrt(diff @ diff))
    bound = FIT_MARGIN * FIT_RESIDUAL * condG * float(np.sqrt(b_ref @ b_ref))
    assert err <= bound, "%s: |b - b*| = %.3e > %.3e = 4e-13 * cond (%.3g) * |b*| (%.2f of the bound)" % (
        what, err, bound, condG, err / max(bound, 1e-300))
    return err / max(bound, 1e-300)


def assert_loss_close(got, ref, what):
    """|loss - loss*| <= 2e-10 loss*.  Returns the relative error."""
    ref = LD(ref)
    rel = float(abs(LD(got) - ref) / ref) if ref != 0 else float(abs(LD(got)))
    assert rel <= LOSS_RTOL, "%s: loss %.17g, reference %.17g, relative error %.3e > %.1e" % (
        what, float(got), float(ref), rel, LOSS_RTOL)
    return rel


def assert_gram_close(got, ref, col_norms, row_norms, n, what, extra=None, scale=1.0):
    """Per entry |G_ja - G*_ja| <= 32 sqrt(n) u |x_j| |x_a| (got, ref: p x c; col_norms: |x_a| of the c exported columns,
    row_norms: |x_j| of all p).  extra (p x c, optional): what the caller's inputs carry into each entry, added to the
    bound (tests/glmref.py: the working weights and response are computed quantities); scale: the whole bound times this
    (two results against each other: 2).  Returns the largest fraction of the bound used."""
    bound = GRAM_FACTOR * np.sqrt(float(n)) * U * np.outer(np.asarray(row_norms, float), np.asarray(col_norms, float))
    if extra is not None:
        bound = bound + np.asarray(extra, dtype=np.float64)
    bound = scale * bound
    frac = np.abs((ld(got) - ld(ref)).astype(np.float64)) / bound
    j, a = np.unravel_index(int(np.argmax(frac)), frac.shape)
    assert frac[j, a] <= 1.0, "%s: Gram entry (%d, %d) is off by %.3e = %.2f of 32 sqrt(n) u |x_j||x_a|" % (
        what, j, a, frac[j, a] * bound[j, a], frac[j, a])
    return float(frac[j, a])


def normalization_tolerance(n, x_mean, x_norm):
    """4 sqrt(n) u (1 + |mean_j| / sd_j) per column, sd_j = norm_j / sqrt(n): the conditioning of the subtraction times
    the growth of a length-n sum.  For the entries of a normalised column relative to 1, for x_norm_j relatively."""
    sd = np.asarray(x_norm, dtype=np.float64) / np.sqrt(float(n))
    return NORM_FACTOR * np.sqrt(float(n)) * U * (1.0 + np.abs(np.asarray(x_mean, dtype=np.float64)) / sd)


def assert_normalization_close(Xs, xm, xn, ref, w, what):
    """Columns (relative to 1, their size after scaling; weighted rows relative to sqrt(w_i)), x_norm relatively, x_mean
    relative to sd + |mean| u -- all within normalization_tolerance of the longdouble reference (Xn, yn, xm, xn, ym).
    Returns the largest fraction of the tolerance used by (columns, x_norm)."""
    Xr, _, xmr, xnr, _ = ref
    n = Xr.shape[0]
    tol = normalization_tolerance(n, xmr, xnr)
    scale = np.sqrt(np.asarray(w, dtype=np.float64))[:, None]
    fc = np.max(np.abs((ld(Xs) - Xr).astype(np.float64)) / scale, axis=0) / tol
    fn = np.abs(((ld(xn) - xnr) / xnr).astype(np.float64)) / tol
    sd = xnr.astype(np.float64) / np.sqrt(float(n))
    fm = np.abs((ld(xm) - xmr).astype(np.float64)) / (tol * sd)
    j = int(np.argmax(fc))
    assert fc[j] <= 1.0, "%s: column %d off by %.2f of 4 sqrt(n) u (1 + |mean|/sd) = %.3e" % (what, j, fc[j], tol[j])
    j = int(np.argmax(fn))
    assert fn[j] <= 1.0, "%s: x_norm[%d] off by %.2f of the tolerance %.3e" % (what, j, fn[j], tol[j])
    j = int(np.argmax(fm))
    assert fm[j] <= 1.0, "%s: x_mean[%d] off by %.2f of the tolerance %.3e sd" % (what, j, fm[j], tol[j])
    return float(fc.max()), float(fn.max())


def ic_value(train_loss, n, p, T0, ic_type):
    """LmMetric::ic for singleton groups (src/Metric.h:205-229): n log(loss) + c T0."""
    c = {1: 2.0, 2: np.log(n), 3: np.log(p) * np.log(np.log(n)), 4: np.log(n) + 2.0 * np.log(p)}[ic_type]
    return float(n * np.log(LD(train_loss)) + c * T0)


# ---- seeded inputs, one place for both files -------------------------------------------------------------------------
SNR_LEVELS = (1e-3, 3e-6, 1e-6, 3e-7, 1e-9, 1e-13)  # tr / yy at the true support; 1e-6 is the library's guard
GRAM_SHAPES = [(n, p) for n in (130, 1023, 1025, 3001) for p in (33, 127, 129, 1100)]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def weights(n, seed=5):
    """Non-unit observation weights that sum to n (the reference's formulas divide by n, not by sum(w))."""
    w = _rng(seed).uniform(0.25, 1.75, n)
    return w * (n / w.sum())


def folds(n, K=4, seed=17):
    return _rng(seed).permutation(n).astype(np.int32) % K


def design_iid(n=3001, p=1300, k_true=40, seed=101):
    """make_lm-like: N(0,1) columns, coefficients 5 sqrt(2 log p / n) U(1, 100) with random signs, N(0,1) noise."""
    rng = _rng(seed)
    X = rng.standard_normal((n, p))
    sup = np.sort(rng.choice(p, k_true, replace=False))
    b = 5.0 * np.sqrt(2.0 * np.log(p) / n) * rng.uniform(1.0, 100.0, k_true) * rng.choice([-1.0, 1.0], k_true)
    return X, X[:, sup] @ b + rng.standard_normal(n), sup


def design_ar1(n=3001, p=1300, k_true=40, rho=0.9, seed=102):
    """Correlated columns: x_j = rho x_{j-1} + sqrt(1 - rho^2) z_j.  Conjugate gradients need many more than 8 steps."""
    rng = _rng(seed)
    Z = rng.standard_normal((n, p))
    X = np.empty((n, p))
    X[:, 0] = Z[:, 0]
    c = np.sqrt(1.0 - rho * rho)
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + c * Z[:, j]
    sup = np.sort(rng.choice(p, k_true, replace=False))
    b = 5.0 * np.sqrt(2.0 * np.log(p) / n) * rng.uniform(1.0, 100.0, k_true) * rng.choice([-1.0, 1.0], k_true)
    return X, X[:, sup] @ b + rng.standard_normal(n), sup


def design_collinear(seed=11):
    """6 clusters of 50 almost equal columns (tests/test_cov_gpu.py): conjugate gradients miss the residual target."""
    rng = _rng(seed)
    n, p = 1500, 300
    z = rng.standard_normal((n, 6))
    X = np.repeat(z, 50, axis=1) + 1e-4 * rng.standard_normal((n, p))
    return X, X[:, 0] - 2 * X[:, 60] + 1.5 * X[:, 130] + rng.standard_normal(n), np.array([0, 60, 130])


def design_snr(level, n=3001, p=300, k_true=10, seed=103):
    """The iid design with the noise scaled so that |y - X_S b|^2 / |y|^2 at the true support S is about `level`."""
    rng = _rng(seed)
    X = rng.standard_normal((n, p))
    sup = np.sort(rng.choice(p, k_true, replace=False))
    b = rng.uniform(1.0, 3.0, k_true) * rng.choice([-1.0, 1.0], k_true)
    s = X[:, sup] @ b
    s0 = s - s.mean()
    sigma = np.sqrt(level * (s0 @ s0) / (n - k_true - 1))
    return X, s + sigma * rng.standard_normal(n), sup


def design_large_mean(n, p, seed=104, fp32_exact=False):
    """Column j = 1e6 + 10^(j mod 7 - 3) N(0,1): a spread of scales and means up to 1e9 standard deviations.
    fp32_exact: every value representable in fp32 (mean 2^20, deviations rounded to quarters (2^-2; the fp32 spacing at 2^20 is 2^-3) of Z times the column's scale >= 1),
    so that widening an fp32 source is exact."""
    rng = _rng(seed + 1000 * n + p)
    Z = rng.standard_normal((n, p))
    if fp32_exact:
        X = 2.0 ** 20 + np.round(Z * 10.0 ** (np.arange(p) % 3) * 4.0) / 4.0
        X = X.astype(np.float32).astype(np.float64)
    else:
        X = 1e6 + Z * 10.0 ** (np.arange(p) % 7 - 3.0)
    y = rng.standard_normal(n) + 3.0
    return X, y


def designs():
    """Name -> (X, y, true support) of every design the precision tests use, built lazily."""
    d = {"iid": design_iid, "ar1": design_ar1, "ar03": (lambda: design_ar1(rho=0.3, seed=106)), "collinear": design_collinear}
    for lv in SNR_LEVELS:
        d["snr%g" % lv] = (lambda lv=lv: design_snr(lv))
    return d
