"""Reference side of the score-state tests (tests/test_score_state_reference.py on the CPU, tests/test_score_state_gpu.py
on the GPU): the cases both files walk, the two helpers the state needs beyond tests/xprec.py -- block_extremes (exact) and
residual (longdouble) -- and the exact consistency checks of a state record, written against plain dictionaries so that
the CPU file can feed them broken ones.  Scores themselves go through xprec.scores / xprec.score_error_units.

A state record is what bess_amd.capi.Session.score_state returns: the control block's fields, the host's record of the
fit it describes ("row_set", "lambda", "bmm_owner", "known"), A_cur, b_cur, beta_dense, inA, bd, the sums bd was formed
from ("d", or "part" and "r") and the per-block extremes bmm_min / bmm_max / bmm_arg."""
import numpy as np

import xprec

LD = np.longdouble
DBL_MAX = float(np.finfo(np.float64).max)
NO_COLUMN = 2147483647  # what k_cov_d leaves as the arg-max of a block without a column outside the active set

# ---- the cases (smallest shapes at which the kernels can go wrong) ----------------------------------------------------------
# n -> (U, nrb) of the streaming pass: row blocks of 128 U rows; nrb = 8 fills k_score's four groups evenly, 2 and 5 do not
GEOMETRY = {130: (1, 2), 1023: (1, 8), 1025: (2, 5), 2049: (4, 5), 4097: (8, 5)}
# p: one column past a 32-block of k_cov_d, a 64-block of k_score, a column group of k_xtv
SWEEP = [(kind, n, p) for kind in ("iid", "ar1") for n in sorted(GEOMETRY) for p in (33, 65, 129)]
T0S, LAMS, FOLDS = (1, 8, 33), (0.0, 0.3), (-1, 0)
SNR_SHAPE = {"n": 1025, "p": 65, "k_true": 6}
WIDE = ("iid", 1025, 1100)          # k_cur > 64
WIDE_T0 = 100
CHUNKED = ("iid", 2049, 1100)       # a level above the CHUNK = 512 staging of cov_d_body
CHUNKED_T0, CHUNKED_LAM = 520, 0.3


# Seeds.  A fit that ends on a CYCLE of active sets (or, at level 1, on column 0: the all-zero first column of A_list) leaves
# scores of the coefficients before its last solve (d_fresh = 0), which nothing can be compared with.  Every fit of the sweep
# must end on the set of the iteration before; tests/test_score_state_reference.py shows with the fp64 restatement that it
# does for these seeds (101 unless listed: the first seed from 101 up for which all 24 fits of the case do).
SEEDS = {("iid", 1023, 33): 102, ("iid", 1023, 129): 103, ("iid", 2049, 129): 103, ("iid", 4097, 33): 102,
         ("iid", 4097, 129): 103, ("ar1", 1023, 65): 102, ("ar1", 1025, 33): 102, ("ar1", 2049, 33): 102,
         ("ar1", 4097, 129): 103}


def make_design(kind, n, p):
    """(X, y, true support, weights): the sweep designs carry non-unit weights, the SNR designs (kind = "snr<level>") none."""
    if kind.startswith("snr"):
        X, y, sup = xprec.design_snr(float(kind[3:]), **SNR_SHAPE)
        return X, y, sup, np.ones(len(y))
    X, y, sup = (xprec.design_iid if kind == "iid" else xprec.design_ar1)(n, p, k_true=8, seed=SEEDS.get((kind, n, p), 101))
    return X, y, sup, xprec.weights(n)


def tied_pair(sup):
    """The two columns of block 1 (32..63) that tie_columns makes equal: the first two outside the true support."""
    out = np.setdiff1d(np.arange(32, 64), sup)
    return int(out[0]), int(out[1])


def tie_columns(X, y, sup):
    """Two bitwise equal columns outside the support whose common score is the largest outside it in their block: the
    second is a copy of the first, and the response gets a small share of it (0.3 against true coefficients >= 0.45 and a
    noise level of n^-1/2 in the score)."""
    lo, hi = tied_pair(sup)
    X = X.copy()
    X[:, hi] = X[:, lo]
    return X, y + 0.3 * X[:, lo]


# (e): fits that take every branch of the covariance form's slot on ONE session, in order: (what, T0, lambda, fold, index of
# the earlier fit whose model it starts from or None, empty the session first)
SEQUENCE = [
    # the arg-max start: level k, then k + 1 and k + 2 from the device's own state, at the same lambda
    ("grow1 k", 8, 0.0, -1, None, True), ("grow1 k+1", 9, 0.0, -1, 0, False), ("grow1 k+2", 10, 0.0, -1, 1, False),
    ("grow1 k, lambda 0.3", 8, 0.3, -1, None, True), ("grow1 k+1, lambda 0.3", 9, 0.3, -1, 3, False),
    ("grow1 k+2, lambda 0.3", 10, 0.3, -1, 4, False),
    # the lambda-only re-score (k_score with nrb = 1): the same level at lambda 0, 0.3, 0; then the chained start
    ("lambda 0", 8, 0.0, -1, None, True), ("lambda 0 -> 0.3", 8, 0.3, -1, 6, False), ("lambda 0.3 -> 0", 8, 0.0, -1, 7, False),
    ("lambda 0 again: nothing is recomputed", 8, 0.0, -1, 8, False),
    # a row-set switch: bd is one buffer for all row sets, nothing may be kept across the switch
    ("fold 0", 8, 0.0, 0, None, True), ("fold 0 -> all rows", 8, 0.0, -1, 10, False), ("all rows -> fold 0", 8, 0.0, 0, 10, False),
    ("fold 0 -> all rows, its own model", 8, 0.0, -1, 11, False),
]
SEQ_CASE = ("iid", 1025, 129)


def fold_mask(n, fold):
    return None if fold < 0 else xprec.folds(n) != fold


def walk_fits(fit):
    """The fits of one sweep session, in order.  fit(fold, lam, T0, start) runs one (start = None: cold, from an emptied
    session; else the record of the model to start from) and returns a record with "support" and "beta".  A warm fit starts
    from the cold model of the level before (at the first level: from its own cold model, which the device still holds).
    Yields (fold, lam, T0, "cold" | "warm", record)."""
    for fold in FOLDS:
        for lam in LAMS:
            prev = None
            for T0 in T0S:
                cold = fit(fold, lam, T0, None)
                yield fold, lam, T0, "cold", cold
                yield fold, lam, T0, "warm", fit(fold, lam, T0, cold if prev is None else prev)
                prev = cold


N_FITS = len(FOLDS) * len(LAMS) * len(T0S) * 2
# the two fits built to end with d_fresh == 0: out of iterations after one solve, and after two that did not repeat
LIMITED = ("ar1", 1025, 65)
LIMITED_T0 = 8


# ---- helpers -------------------------------------------------------------------------------------------------------------
def block_extremes(bd, A, p, block=32):
    """Per block of 32 columns, exactly (min and max commute with rounding): the smallest bd over the block's columns in A
    (DBL_MAX if none), the largest over the others (-1.0 if none) and the lowest column attaining that maximum (NO_COLUMN
    if none).  always_select columns need no special case: their bd is DBL_MAX already, inside A or outside it, which is
    how k_cov_d treats them."""
    bd = np.asarray(bd, dtype=np.float64)
    assert bd.shape == (p,)
    inside = np.zeros(p, dtype=bool)
    inside[np.asarray(A, dtype=int)] = True
    nb = (p + block - 1) // block
    mn, mx, arg = np.full(nb, DBL_MAX), np.full(nb, -1.0), np.full(nb, float(NO_COLUMN))
    for b in range(nb):
        j = np.arange(b * block, min(p, (b + 1) * block))
        if inside[j].any():
            mn[b] = bd[j[inside[j]]].min()
        out = j[~inside[j]]
        if out.size and bd[out].max() > -1.0:
            mx[b] = bd[out].max()
            arg[b] = float(out[np.argmax(bd[out] == mx[b])])  # (argmax of a boolean array: its first True)
    return mn, mx, arg


def residual(Xn, y, mask, A, b):
    """r = m o (y - X_A b) in longdouble and the elementwise magnitude |y_i| + sum_a |x_ia b_a| (fp64) its fp64 evaluation
    is judged by.  Rows outside the mask are exactly zero in both."""
    A = np.asarray(A, dtype=int)
    X = np.asarray(Xn)[:, A]
    m = np.ones(X.shape[0], dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    r = np.where(m, xprec.ld(y) - xprec.ld(X) @ xprec.ld(b), LD(0))
    mag = np.where(m, np.abs(np.asarray(y, dtype=np.float64)) + np.abs(X.astype(np.float64)) @ np.abs(np.asarray(b, dtype=np.float64)), 0.0)
    return r, mag


def residual_error_units(r_got, r_ref, mag):
    """max_i |r_i - r*_i| / (u magnitude_i); a non-zero entry where the magnitude is zero (a masked row) counts as inf."""
    err = np.abs((xprec.ld(r_got) - r_ref).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(mag > 0, err / (xprec.U * mag), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    return float(ratio[i]), i


def partial_sum_error_units(part, Xn, r_dev):
    """The row-block partials of the streaming pass, added in longdouble, against X^T r_dev in longdouble for the DEVICE's
    own residual: max_j |sum_rb part[rb][j] - x_j.r_dev| / (u sum_i |x_ij r_i|).  Returns (largest ratio, its column)."""
    X = np.asarray(Xn, dtype=np.float64)
    got = xprec.ld(part).sum(axis=0)
    want = xprec.ld(X).T @ xprec.ld(r_dev)
    room = xprec.U * (np.abs(X).T @ np.abs(np.asarray(r_dev, dtype=np.float64)))
    ratio = np.abs((got - want).astype(np.float64)) / np.maximum(room, 1e-300)
    j = int(np.argmax(ratio))
    return float(ratio[j]), j


def score_units(bd, ref, form, always=()):
    """xprec.score_error_units over the columns that are not always_select; those must be exactly DBL_MAX."""
    bd = np.asarray(bd, dtype=np.float64)
    al = np.asarray(always, dtype=int)
    assert np.all(bd[al] == DBL_MAX), "always_select scores are not DBL_MAX: %r" % (bd[al],)
    if al.size:
        keep = np.setdiff1d(np.arange(bd.size), al)
        sub = {k: np.asarray(v)[keep] for k, v in ref.items()}
        c, j = xprec.score_error_units(bd[keep], sub, form)
        return c, int(keep[j])
    return xprec.score_error_units(bd, ref, form)


# ---- exact checks of a state record (4a, 4d) ------------------------------------------------------------------------------
def assert_state_consistent(st, returned=None, what=""):
    """beta_dense[A_cur] == b_cur and zero elsewhere; A_cur without repeats; inA exactly the membership of A_cur (where the
    session keeps the flags); after a committed solve k_cur == T0; with `returned` (a fit record) and done && d_fresh,
    A_cur / b_cur are the support and coefficients the call returned, bit for bit."""
    A, b, p = np.asarray(st["A_cur"]), np.asarray(st["b_cur"]), len(st["beta_dense"])
    assert len(A) == st["k_cur"] == len(b), "%s: k_cur = %d, %d indices, %d coefficients" % (what, st["k_cur"], len(A), len(b))
    assert np.all((A >= 0) & (A < p)) and len(np.unique(A)) == len(A), "%s: A_cur is not a set of columns: %r" % (what, A)
    dense = np.zeros(p)
    dense[A] = b
    assert np.array_equal(st["beta_dense"], dense), "%s: beta_dense is not b_cur scattered to A_cur (columns %r)" % (
        what, np.nonzero(st["beta_dense"] != dense)[0][:8])
    if st["has_inA"]:
        member = np.zeros(p, dtype=bool)
        member[A] = True
        assert np.array_equal(np.asarray(st["inA"], dtype=bool), member), "%s: inA differs from the membership of A_cur at %r" % (
            what, np.nonzero(np.asarray(st["inA"], dtype=bool) != member)[0][:8])
    if st["l"] >= 1:
        assert st["k_cur"] == st["T0"], "%s: k_cur = %d after a committed solve of level %d" % (what, st["k_cur"], st["T0"])
    if returned is not None and st["done"] and st["d_fresh"]:
        assert np.array_equal(A, returned["support"]), "%s: A_cur %r is not the returned support %r" % (what, A, returned["support"])
        assert np.array_equal(b, returned["beta"]), "%s: b_cur is not the returned coefficients" % what


def assert_block_extremes(st, what=""):
    """cov_bmm == block_extremes(bd, A_cur, p), exactly, from the device's own bd."""
    p = len(st["bd"])
    mn, mx, arg = block_extremes(st["bd"], st["A_cur"], p)
    for got, want, name in ((st["bmm_min"], mn, "minimum inside"), (st["bmm_max"], mx, "maximum outside"),
                            (st["bmm_arg"], arg, "column of the maximum outside")):
        bad = np.nonzero(np.asarray(got) != want)[0]
        assert bad.size == 0, "%s: block %d: %s the active set is %r, bd says %r" % (what, bad[0] if bad.size else -1, name,
                                                                                      np.asarray(got)[bad[:1]], want[bad[:1]])


# ---- fp64 NumPy restatement of one fit (which listed fits end on a repeated set; the synthetic states of the CPU file) --
def pdas_fit(Xn, y, mask, T0, lam, init_idx=(), init_val=(), max_iter=20, always=()):
    """Algorithm::fit for LM with singleton groups in fp64 NumPy (ties at the selection boundary: lower column first).
    Returns {"A", "b", "bd", "iters", "end"}: end = "repeat" (the set of the iteration before: the device ends done with
    d_fresh = 1), "cycle" (an earlier set: done, d_fresh = 0) or "iterations" (max_iter reached); bd are the scores the
    LAST iteration ranked."""
    X = np.asarray(Xn, dtype=np.float64)
    n, p = X.shape
    m = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    Xt, yt = X[m], np.asarray(y, dtype=np.float64)[m]
    nt = float(m.sum())
    phi = np.sqrt(2 * lam + (Xt * Xt).sum(axis=0) / nt)
    beta = np.zeros(p)
    beta[np.asarray(init_idx, dtype=int)] = np.asarray(init_val, dtype=np.float64)
    seen, end, A, bA, bd = [np.zeros(T0, dtype=np.int64)], "iterations", None, None, None
    for it in range(1, max_iter + 1):
        d = Xt.T @ (yt - Xt @ beta) / nt - 2 * lam * beta
        bd = (phi * beta + d / phi) ** 2
        bd[np.asarray(always, dtype=int)] = DBL_MAX
        A = np.sort(np.lexsort((np.arange(p), -bd))[:T0])
        if it >= 2 and np.array_equal(A, seen[-1]):
            end = "repeat"
            break
        bA = np.linalg.solve(Xt[:, A].T @ Xt[:, A] + lam * np.eye(T0), Xt[:, A].T @ yt)
        beta = np.zeros(p)
        beta[A] = bA
        hit = any(np.array_equal(A, a) for a in seen)
        seen.append(A)
        if hit:
            end = "cycle"
            break
    return {"A": A, "b": bA, "bd": bd, "iters": it, "end": end}
