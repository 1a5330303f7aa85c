"""Extended-precision reference and error bounds for bessx_info_device / bess_base.inference (shared by
tests/test_info_api.py and tests/test_info_gpu.py, in the manner of tests/evalref.py and tests/coxevalref.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values, eta* and its per-row bound Delta_i from
evalref.eta_reference (the eta arithmetic is that of bessx_k_xb.hpp, unchanged, so that analysis carries over):

    z_i = (1, x(i, cols[0]), ...),    I* = sum_i v*_i z_i z_i^T,    U* = sum_i g*_i z_i,
    identity  v = w                g = w (y - eta)
    logistic  v = w p (1 - p)      g = w (y - p),   p = 1 / (1 + exp(-eta))
    Poisson   v = w exp(eta)       g = w (y - exp(eta))

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).  Operations as built (bessx_k_info.hip;
bess_base._information_host does the same operations in fp64 NumPy):

1. Row factor rf_i, the relative error of v_i.  |d log v / d eta| <= 1 for the logistic link (v = t / (1 + t)^2 with
   t = exp(-|eta|): d log v / d log t = (1 - t) / (1 + t)) and = 1 for Poisson, so evaluating at eta_hat instead of eta*
   costs a factor within exp(+-Delta_i); then the roundings:
       identity   v = w, no operation:                                                rf = 0
       logistic   exp: 1 ulp = 2 u;  s = 1 + t enters squared: 2 u;  s * s: u;  t / (s s): u;  w * (.): u
                                                                                      rf = expm1(Delta) + exp(Delta) gamma_7
       Poisson    exp: 2 u;  w * e: u                                                 rf = expm1(Delta) + exp(Delta) gamma_3
2. Score weight, absolute: dmu_i bounds |mu_hat - mu*|,
       identity   dmu = Delta
       logistic   |d log p / d eta| = 1 - p <= 1: exp 2 u, s = 1 + t u, the quotient u
                                                  dmu = p* (expm1(Delta) + exp(Delta) gamma_4)
       Poisson    dmu = e* (expm1(Delta) + exp(Delta) gamma_2)
   then y - mu (one rounding) and w * (.) (one):  dg_i = w_i (dmu_i + gamma_2 (|y_i - mu*_i| + dmu_i)).
3. Sums.  An entry of I is sum_i a_i b_i with a = z_ij exact, b = z_ik * v_hat_i (one rounding), the product inside the
   matrix instruction (at most one) and an addition chain of length `depth`: any order of additions of that length obeys
   gamma_depth (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  On the device a wave adds the
   rows of its slab (rows_per_slab terms, however the instruction orders the four products of an issue), k_info_finish
   adds ceil(slabs / 16) partials per lane in slab order and then 4 levels of the DPP tree:
       depth_device = rows_per_slab + ceil(slabs / 16) + 4       (device_depth(): the split comes from the library)
   and the NumPy route is a matrix product over n rows: depth_host = n.
       |I_jk - I*_jk| <= sum_i v*_i |z_ij z_ik| (rf_i + (1 + rf_i) gamma_{depth + 2})
       |U_j  - U*_j | <= sum_i |z_ij| (dg_i + (|g*_i| + dg_i) gamma_{depth + 1})
4. Self-check: the bound on I, as a multiple of sum_i v*_i |z_ij z_ik|, must stay below REL_CEILING = 1e-9 for every
   input a test uses (the ceiling of tests/coxsurvref.py); information_reference asserts it, so a bound cannot grow
   quietly until it hides a failure.
5. Standard errors.  With D* = diag(I*)^(-1/2) and S* = D* I* D*, the computed matrix is S* + E with |E_jk| <= r (the
   relative entry bound of step 4 and Cauchy-Schwarz: sum_i v |z_ij z_ik| <= sqrt(I_jj I_kk)), so ||E||_2 <= M r.  To
   first order the change of (S^-1)_jj is e_j^T S^-1 E S^-1 e_j <= ||E||_2 (S^-2)_jj <= ||E||_2 (S^-1)_jj / lambda_min,
   and 1 / lambda_min <= cond(S*) because lambda_max >= 1 for a unit diagonal.  The fp64 factorisation and solves of
   wald_table add a backward error of at most 8 M^2 u in the same norm (Higham, theorem 10.4 with its constant
   rounded up).  A factor 2 covers the second-order terms while cond(S*) (M r + 8 M^2 u) < 0.1, which se_bound
   asserts together with cond(S*) < 1e6; se is a square root (half the relative error) and, for the identity link,
   carries half the relative error of the dispersion loss / (sum_w - M), i.e. of evalref's loss bound:
       |se - se*| / se* <= cond(S*) (M r + 8 M^2 u) + loss_bound / (2 loss*)."""
import numpy as np

import evalref

LD = evalref.LD
U = evalref.U
gamma = evalref.gamma
REL_CEILING = LD(1e-9)
COND_CEILING = 1e6


def device_depth(capi, n, m):
    """depth_device of step 3 for an n-row call with m support columns: the split is the library's own figure."""
    _, rps, slabs = capi.info_workspace(n, m)
    return int(rps) + (int(slabs) + 15) // 16 + 4


def information_reference(vals, cols, beta, c, y, w, link, depth):
    """Reference and bounds of one call.  vals: the (widened) n x p values; cols, beta (m,), c; y (n,), w (n,) or None;
    depth: the addition chain of step 3.  Returns longdouble arrays: info, info_bound (M, M), score, score_bound (M,),
    sum_v, rel (the largest info_bound / sum_i v |z z|), plus evalref's loss reference under "loss"."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    n, m = np.asarray(vals).shape[0], cols.size
    eta, delta = evalref.eta_reference(vals, cols, np.asarray(beta, dtype=np.float64).reshape(m, 1), [c])
    loss = evalref.loss_reference(eta, delta, y, w, link)
    eta, delta = eta[:, 0], delta[:, 0]
    yl = np.asarray(y).astype(LD).reshape(-1)
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)
    grow = np.exp(delta)
    if link == "identity":
        mu, v, rf, dmu = eta, wl.copy(), np.zeros(n, dtype=LD), delta
    elif link == "logistic":
        mu = LD(1) / (LD(1) + np.exp(-eta))
        v = wl * mu * (LD(1) / (LD(1) + np.exp(eta)))
        rf = np.expm1(delta) + grow * gamma(7)
        dmu = mu * (np.expm1(delta) + grow * gamma(4))
    elif link == "poisson":
        mu = np.exp(eta)
        v = wl * mu
        rf = np.expm1(delta) + grow * gamma(3)
        dmu = mu * (np.expm1(delta) + grow * gamma(2))
    else:
        raise ValueError(link)
    g = wl * (yl - mu)
    dg = wl * (dmu + gamma(2) * (np.abs(yl - mu) + dmu))
    # (Z^T as a contiguous array: NumPy's longdouble products have no BLAS behind them and are slow on strided operands.
    # The bounds themselves are sums of non-negative terms: fp64 BLAS forms them to a relative gamma_n, far inside the
    # 2^-20 by which they are enlarged here.)
    Zt = np.ascontiguousarray(np.concatenate([np.ones((n, 1), dtype=LD), np.asarray(vals)[:, cols].astype(LD)], axis=1).T)
    At = np.abs(Zt).astype(np.float64)
    up = LD(1) + LD(2.0) ** -20
    info = np.einsum("ji,ki->jk", Zt * v[None, :], Zt)
    info = np.tril(info) + np.tril(info, -1).T
    mass = ((At * v.astype(np.float64)[None, :]) @ At.T).astype(LD)
    info_bound = ((At * (v * (rf + (LD(1) + rf) * gamma(depth + 2))).astype(np.float64)[None, :]) @ At.T).astype(LD) * up
    score = Zt @ g
    score_bound = np.abs(Zt) @ (dg + (np.abs(g) + dg) * gamma(depth + 1))
    pos = mass > 0
    rel = (info_bound[pos] / mass[pos]).max() if pos.any() else LD(0)
    assert rel < REL_CEILING, ("the derived bound exceeds its ceiling: choose other inputs", float(rel))
    return {"info": info, "info_bound": info_bound, "score": score, "score_bound": score_bound, "sum_v": v.sum(),
            "rel": rel, "loss": loss, "M": m + 1, "link": link}


def check_information(got, ref, what=""):
    """Print the figures, then assert info and score against their bounds."""
    gi, gs = np.asarray(got["info"]).astype(LD), np.asarray(got["score"]).astype(LD)
    ei, es = np.abs(gi - ref["info"]), np.abs(gs - ref["score"])
    wi = np.unravel_index(int(np.argmax(ei - ref["info_bound"])), ei.shape)
    ws = int(np.argmax(es - ref["score_bound"]))
    print("%s: info err %.3e against bound %.3e at %s; score err %.3e against bound %.3e at %d" % (
        what, float(ei[wi]), float(ref["info_bound"][wi]), wi, float(es[ws]), float(ref["score_bound"][ws]), ws))
    assert np.isfinite(np.asarray(got["info"])).all() and np.isfinite(np.asarray(got["score"])).all(), what
    assert (ei <= ref["info_bound"]).all(), (what, wi, float(ei[wi]), float(ref["info_bound"][wi]))
    assert (es <= ref["score_bound"]).all(), (what, ws, float(es[ws]), float(ref["score_bound"][ws]))


def ld_inverse_spd(A):
    """Inverse of a symmetric positive definite longdouble matrix by Cholesky (numpy.linalg has no longdouble)."""
    A = np.array(A, dtype=LD)
    M = A.shape[0]
    L = np.zeros((M, M), dtype=LD)
    for j in range(M):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        assert d > 0, "the reference matrix is not positive definite"
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.zeros((M, M), dtype=LD)  # L Y = I
    for j in range(M):
        rhs = np.zeros(M, dtype=LD)
        rhs[j] = LD(1)
        Y[j] = (rhs - L[j, :j] @ Y[:j]) / L[j, j]
    return Y.T @ Y


def se_reference(ref):
    """(se*, cov*, relative bound on se, cond(S*)) of a reference from information_reference.  Asserts step 5's
    preconditions: cond(S*) < 1e6 and cond(S*) (M r + 8 M^2 u) < 0.1."""
    I, M = ref["info"], ref["M"]
    d = LD(1) / np.sqrt(np.diag(I))
    S = I * d[:, None] * d[None, :]
    ev = np.linalg.eigvalsh(S.astype(np.float64))
    cond = float(ev[-1] / ev[0])
    assert cond < COND_CEILING, ("cond(S*) is too large for the se bound: choose other inputs", cond)
    cov = ld_inverse_spd(S) * d[:, None] * d[None, :]
    rel = LD(cond) * (LD(M) * ref["rel"] + LD(8 * M * M) * U)
    assert rel < LD(0.1), float(rel)
    if ref["link"] == "identity":
        L = ref["loss"]
        dof = L["sum_w"] - LD(M)
        cov = cov * (L["loss"][0] / dof)
        rel = rel + L["bound"][0] / (LD(2) * L["loss"][0])
    return np.sqrt(np.diag(cov)), cov, rel, cond
