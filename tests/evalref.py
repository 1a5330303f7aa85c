"""Extended-precision reference and error bound for the held-out losses of bessx_eval_device / bess_base.evaluate
(shared by tests/test_eval_api.py and tests/test_eval_gpu.py, in the manner of tests/xprec.py).

Reference: NumPy in np.longdouble on the host copy of the same (widened) values:

    eta*(i, r) = sum_k x(i, cols[k]) B[k, r] + c_r,        L*_r = sum_i w_i f(eta*(i, r), y(i, r)).

(On x86 longdouble carries 64 significant bits; the reference's own error is 2^-11 of every figure below and is not
added.)

The bound is derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).

1. Linear predictor (the bound of tests/test_predict_gpu.py; Higham, Accuracy and Stability of Numerical Algorithms,
   section 3.1: an m-term dot product plus one addition, any order, with or without fused multiply-add):
       |eta_hat - eta*| <= Delta_i = gamma_{m+2} (|c_r| + sum_k |x_ik| |B_kr|).
2. The row's term f is evaluated at eta_hat instead of eta*: |f(eta_hat) - f(eta*)| <= Lip_i Delta_i with Lip_i the
   largest |df/deta| on eta* +- Delta_i:
       identity   (y - a)^2 - (y - b)^2 = (b - a) (2 (y - b) - (a - b)), so Lip_i = 2 |y - eta*| + Delta_i
       logistic   |sigmoid(eta) - y| <= 1 for y in [0, 1]
       Poisson    |exp(eta) - y|                 <= |y| + exp(eta* + Delta_i)
3. q_i, the rounding of the term's own operations in fp64, each operation counted once (a fused multiply-add only
   removes one of them).  Magnitudes are taken at |eta*| + Delta_i.
       identity   d = y - eta (1 rounding), d * d (1): relative (1 + u)^3 - 1 <= gamma_3 on d^2:
                  q = gamma_3 (|y - eta*| + Delta_i)^2
       logistic   e = exp(-|eta|): 1 ulp = 2 u relative, e <= 1; log1p propagates it with slope <= 1: 2 u e
                  log1p itself: an ALLOWANCE of 4 u log 2 (not a derived figure: the accuracy of the device's and of
                  NumPy's log1p is documented as "a few ulp", and log1p(e) <= log 2)
                  s = max(eta, 0) + log1p(e) (1 rounding): u s;  t = y * eta (1): u |y eta|;  s - t (1): u (s + |y eta|)
                  q = u (4 log 2 + 2 e + 2 s + 2 |y| |eta|)
       Poisson    e = exp(eta): 1 ulp = 2 u e;  t = y * eta (1): u |y eta|;  e - t (1): u (e + |y eta|)
                  q = u (3 e + 2 |y| |eta|)
4. The weighted sum: one multiplication by w_i and n - 1 additions, in any order: gamma_n sum_i |w_i f_i|.

Together, as the issue of this feature states it,

    |L_hat_r - L*_r| <= sum_i w_i (Lip_i Delta_i + q_i) + gamma_n sum_i |w_i f_i|.

The weighted count of correct labels A_r involves no rounding of the predictor once no row has |eta*| <= Delta_i (the
sign of eta_hat is then the sign of eta*) and no row has y = 0.5; it is a sum of weights and must EQUAL the reference
when the weights are such that their partial sums are exact (the tests use weights that are multiples of 1/8), else it is
within gamma_n sum_i w_i.  label_precondition() asserts the two conditions; the tests call it for every case.
sum_w: within gamma_n sum_i |w_i| of the reference, exactly n without weights."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
LOG2 = np.log(LD(2.0))


def gamma(k):
    k = LD(k) * U
    return k / (LD(1) - k)


def eta_reference(vals, cols, B, c):
    """(eta*, Delta) in longdouble for the (widened) values of the view, both (n, R)."""
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    Xs = np.asarray(vals)[:, cols].astype(LD)
    cl = np.asarray(c, dtype=LD).reshape(-1)
    Bl = np.asarray(B, dtype=LD).reshape(cols.size, cl.size)
    eta = Xs @ Bl + cl[None, :]
    delta = gamma(cols.size + 2) * (np.abs(Xs) @ np.abs(Bl) + np.abs(cl)[None, :])
    return eta, delta


def loss_reference(eta, delta, y, w, link):
    """Reference and bound for one call: eta, delta (n, R) from eta_reference; y (n,) / (n, 1) shared or (n, R); w (n,)
    or None; link "identity" / "logistic" / "poisson".  Returns a dict of longdouble arrays: loss (R,), bound (R,),
    correct (R,) (logistic, else None), sum_w, sum_w_bound, and labels_ok (n, R) bool: |eta*| > Delta and y != 0.5."""
    n, R = eta.shape
    Y = np.asarray(y).astype(LD).reshape(n, -1)
    if Y.shape[1] not in (1, R):
        raise ValueError("y must have 1 or R columns")
    wl = np.ones(n, dtype=LD) if w is None else np.asarray(w).astype(LD).reshape(-1)
    W = wl[:, None]
    mag = np.abs(eta) + delta  # |eta| wherever a magnitude is needed
    if link == "identity":
        d = np.abs(Y - eta)
        f = (Y - eta) ** 2
        lip = LD(2) * d + delta
        q = gamma(3) * (d + delta) ** 2
    elif link == "logistic":
        e = np.exp(-np.abs(eta))
        f = np.maximum(eta, LD(0)) + np.log1p(e) - Y * eta
        s = np.maximum(eta, LD(0)) + delta + np.log1p(e)
        lip = np.ones_like(eta)
        q = U * (LD(4) * LOG2 + LD(2) * e + LD(2) * s + LD(2) * np.abs(Y) * mag)
    elif link == "poisson":
        f = np.exp(eta) - Y * eta
        e = np.exp(eta + delta)
        lip = np.abs(Y) + e
        q = U * (LD(3) * e + LD(2) * np.abs(Y) * mag)
    else:
        raise ValueError(link)
    loss = (W * f).sum(axis=0)
    bound = (np.abs(W) * (lip * delta + q)).sum(axis=0) + gamma(n) * np.abs(W * f).sum(axis=0)
    out = {"loss": loss, "bound": bound, "correct": None, "sum_w": wl.sum() if w is not None else LD(n),
           "sum_w_bound": gamma(n) * np.abs(wl).sum() if w is not None else LD(0),
           "labels_ok": (np.abs(eta) > delta) & (Y != LD(0.5))}
    if link == "logistic":
        out["correct"] = (W * ((eta > 0) == (Y > LD(0.5)))).sum(axis=0)
    return out


def within(got, ref):
    """Per response: is the computed loss inside the bound of the reference?  (A NaN is never inside.)"""
    got = np.asarray(got).astype(LD).reshape(-1)
    return np.abs(got - ref["loss"]) <= ref["bound"]


def check_loss(got, ref, what=""):
    """Print the figures, then assert the bound for every response."""
    got = np.asarray(got).astype(LD).reshape(-1)
    err = np.abs(got - ref["loss"])
    rel = err / np.maximum(np.abs(ref["loss"]), np.finfo(np.float64).tiny)
    worst = int(np.argmax(err - ref["bound"]))
    print("%s: max rel err %.3e, at the worst response err %.3e against bound %.3e" % (
        what, float(rel.max()), float(err[worst]), float(ref["bound"][worst])))
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), what
    assert (err <= ref["bound"]).all(), (what, worst, float(err[worst]), float(ref["bound"][worst]))


def label_precondition(ref, what=""):
    """The precondition of the exact comparison of `correct`: on EVERY row |eta*| > Delta and y != 0.5."""
    assert ref["labels_ok"].all(), (what, "a row has |eta*| <= Delta or y = 0.5: choose other inputs")
