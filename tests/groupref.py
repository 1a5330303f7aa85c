"""Extended-precision reference for the GROUP-SELECTION kernels reached by bessx_op_group_scores / bessx_op_group_lsq and by
every grouped fit (k_group_moments<2|4|8|16>, k_group_moments_big, k_group_score, k_group_score_big, k_group_lsq_score): pure
NumPy in np.longdouble, no GPU, no oracle.  It restates the formulas AS THE KERNELS STATE THEM (group g = columns
c0 .. c0 + s - 1, X_g its columns, w1 / w2 row weights, ones / absent without):

  moments   mblk_g = X_g' diag(w1) X_g (no division, no ridge),  dcol = X' w2 (left as it was without w2)
  score     M_g = mblk_g (/ n_t with lm) + 2 lam I,  d = dcol (lm: sum over the row blocks of part, / n_t) - 2 lam beta,
            bd_g = |Phi beta_g + Phi^-1 d_g|^2 / s with Phi = sqrtm(M_g)  =  |L' beta_g + L^-1 d_g|^2 / s with M_g = L L'
            (the header comment of k_group_score_big: both are beta'M beta + 2 beta'd + d'M^-1 d); the reference takes the
            Cholesky form with a hand-written longdouble factorisation
  lsq       score_g = |M^-1 d|^2 / s with M = X_g'X_g, d = X_g'yw; a column that depends exactly on the ones before it is
            dropped (coefficient 0, s stays), an all-zero column gives +inf

Bounds.  First-order forward-error expressions evaluated in longdouble from the reference's own values (u = 2^-53):
  moments   xprec's Gram bound, GRAM_FACTOR sqrt(n) u |c_j|_w |c_k|_w with the weighted column norms |c_j|_w =
            sqrt(sum_i |w1_i| x_ij^2); dcol the same with |x_j|_2 |w2|_2.  No constant of this module goes into them.
  score     E_M = the moment bound (/ n_t with lm) + 2 u |M| (the division and the ridge), e_d = the bound of dcol, or
            (nrb + 1) u sum_rb |part| / n_t for lm, + 2 u (|d0| + 2 lam |beta|).  With z = M^-1 d, the first-order change of
            beta'M beta + 2 beta'd + d'M^-1 d is beta'dM beta + 2 beta'dd + 2 z'dd - z'dM z, hence
              carried = |beta|'E_M|beta| + 2 |beta|'e_d + 2 |z|'e_d + |z|'E_M|z|.
            The factorisation (Jacobi or Cholesky) is backward stable: it is exact for M + dM with |dM| of the order
            s u |M|_2, and z'dM z <= |dM|_2 |z|^2 <= |dM|_2 d'M^-1 d / lambda_min, so
              solve = s u cond_2(M) P,  P = beta'M beta + d'M^-1 d + 2 |beta|'|d|  (the score's non-negative summands: where
            L'beta and L^-1 d cancel, the error still is relative to their sizes).
            bound at c = 1: (carried + solve) / s + 4 u bd.
  lsq       dz = M^-1 (dd - dM z), so |z|^2 moves by at most 2 |z|'|M^-1| (e_d + E_M |z|) (|M^-1| entrywise, from the
            longdouble factor), solve = 2 s u cond_2(M) |z|^2; bound at c = 1: (carried + solve) / s + 4 u score.

Constants.  Each score bound is c x (the expression at c = 1).  c is not taken from any kernel: fp64 NumPy evaluating the same
formulas in BOTH forms (eigh-sqrtm and Cholesky: the *_fp64 functions, the CPU stand-in) is measured against this reference on
every case of this module (tests/test_group_reference.py), the maximum is stored as *_NUMPY_MAX and c is the next power of two
at or above four times that (glmref.constant_from); the factor four allows for another valid order of evaluation.  The rule
has no floor: where the Gram bound of the moments dominates the expression (lsq), fp64 NumPy uses a few thousandths of it and
c comes out below 1.  The score check then is tighter on the error the moments carry than assert_moments_close itself is on
the moments: a kernel has to sum as accurately as a pairwise sum does, within the factor four, to pass both.  The GPU has to
fit inside the same constants.

Conditioning.  Scores are compared only where cond_2(M_g) <= COND_LIMIT: beyond it u cond s c passes 1e-2 of the score's
summands and the bound says nothing.  Every case asserts that its groups are under the limit, so none is skipped silently.

The module also owns the seeded cases, so that the CPU and the GPU file use the same inputs."""
import numpy as np

import glmref
import xprec

_frac = glmref._frac
LD, U, EXTENDED = xprec.LD, xprec.U, xprec.EXTENDED
ld = xprec.ld
constant_from = glmref.constant_from
GRP_MAX, TILE = 16, 8  # GRP_MAX of bessx_kdev.hpp, GB_T of k_group_moments_big
DBL_MAX = float(np.finfo(np.float64).max)
COND_LIMIT = 1e11

# fp64 NumPy under the first-order bounds at c = 1: maxima over all_score_cases(), lsq_case() and lsq_short_case() in both
# forms, measured by tests/test_group_reference.py::test_fp64_numpy_sits_inside_every_bound_and_fixes_the_constants (it
# prints them and asserts that they are the ones stored here)
SCORE_NUMPY_MAX = 0.2738   # eigh form, widths up to 8, n = 2, lm, lam = 0.05 (Cholesky form: 0.2152)
LSQ_NUMPY_MAX = 0.0052     # LU solve, n = 3 (Cholesky: 0.0037): the Gram bound of the moments dominates
MOMENT_NUMPY_MAX = 0.0535  # of the Gram bound, whose factor is xprec's: for the record, no constant follows from it
DCOL_NUMPY_MAX = 0.0296    # likewise
SCORE_C = 2.0              # 4 x 0.2738, rounded up to a power of two
LSQ_C = 0.03125            # 4 x 0.0052, rounded up to a power of two


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def layout(gidx, p):
    gidx = np.asarray(gidx, dtype=np.int64).reshape(-1)
    sizes = np.diff(np.concatenate([gidx, [p]]))
    assert gidx[0] == 0 and (sizes > 0).all()
    return gidx, sizes


# ---- longdouble linear algebra, written out (no LAPACK beyond fp64) -----------------------------------------------------------
def chol(M):
    """Lower Cholesky factor of a symmetric positive definite matrix, longdouble, unpivoted."""
    M = ld(M)
    s = M.shape[0]
    L = np.zeros((s, s), dtype=LD)
    for j in range(s):
        v = M[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0, "the reference block is not positive definite"
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def fwd(L, b):
    y = ld(b).copy()
    for j in range(L.shape[0]):
        y[j] = y[j] / L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    return y


def bwd(L, y):
    x = ld(y).copy()
    for j in range(L.shape[0] - 1, -1, -1):
        x[j] = x[j] / L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


# ---- the operations -----------------------------------------------------------------------------------------------------------
def moments(case):
    """mblk (list of longdouble s x s blocks), dcol (longdouble p) and their bounds: norms (|c_j|_w, fp64) for xprec's Gram
    bound, e_dcol (fp64 p; zeros where dcol is an input)."""
    X = np.asarray(case["X"], dtype=np.float64)
    n, p = X.shape
    gidx, sizes = layout(case["gidx"], p)
    Xl = ld(X)
    w1 = np.ones(n, dtype=LD) if case["w1"] is None else ld(case["w1"])
    norms = np.sqrt((np.abs(w1)[:, None] * Xl * Xl).sum(axis=0).astype(np.float64))
    blocks = []
    for c0, s in zip(gidx, sizes):
        Xg = Xl[:, c0:c0 + s]
        blocks.append(Xg.T @ (w1[:, None] * Xg))
    if case["w2"] is not None:
        w2 = ld(case["w2"])
        dcol = Xl.T @ w2
        xn = np.sqrt((Xl * Xl).sum(axis=0).astype(np.float64))
        e_dcol = xprec.GRAM_FACTOR * np.sqrt(float(n)) * U * xn * float(np.sqrt(w2 @ w2))
    else:
        dcol, e_dcol = ld(case["dcol"]), np.zeros(p)
    return {"mblk": blocks, "dcol": dcol, "norms": norms, "e_dcol": e_dcol, "n": n, "p": p, "gidx": gidx, "sizes": sizes}


def scores(case, mom=None):
    """bd of every group in longdouble from the reference moments, with cond_2(M_g) and the bound at c = 1."""
    mom = moments(case) if mom is None else mom
    n, p, gidx, sizes = mom["n"], mom["p"], mom["gidx"], mom["sizes"]
    lam, beta = LD(case["lam"]), ld(case["beta"])
    if case["lm"]:
        part = ld(np.atleast_2d(case["part"]))
        nt = LD(case["n_t"])
        d0 = part.sum(axis=0) / nt
        e_d0 = ((part.shape[0] + 1) * U * np.abs(part).sum(axis=0) / nt).astype(np.float64)
        scale = LD(1) / nt
    else:
        d0, e_d0, scale = mom["dcol"], mom["e_dcol"], LD(1)
    d = d0 - 2 * lam * beta
    e_d = e_d0 + (2 * U * (np.abs(d0) + 2 * lam * np.abs(beta))).astype(np.float64)
    gram1 = xprec.GRAM_FACTOR * np.sqrt(float(n)) * U
    bd, bound, conds, Ms = np.zeros(len(sizes), dtype=LD), np.zeros(len(sizes)), np.zeros(len(sizes)), []
    for g, (c0, s) in enumerate(zip(gidx, sizes)):
        sl = slice(c0, c0 + s)
        M = mom["mblk"][g] * scale + 2 * lam * np.eye(s, dtype=LD)
        Ms.append(M)
        E = gram1 * np.outer(mom["norms"][sl], mom["norms"][sl]) * float(scale) + 2 * U * np.abs(M).astype(np.float64)
        L = chol(M)
        y = fwd(L, d[sl])
        t = L.T @ beta[sl] + y
        z = np.abs(bwd(L, y)).astype(np.float64)
        ab, ad = np.abs(beta[sl]).astype(np.float64), np.abs(d[sl]).astype(np.float64)
        carried = ab @ E @ ab + 2 * ab @ e_d[sl] + 2 * z @ e_d[sl] + z @ E @ z
        P = float(beta[sl] @ M @ beta[sl] + y @ y) + 2 * ab @ ad
        conds[g] = xprec.cond(M)
        bd[g] = (t @ t) / LD(s)
        bound[g] = (carried + s * U * conds[g] * P) / s + 4 * U * float(bd[g])
    return {"bd": bd, "bound": bound, "cond": conds, "M": Ms, "d": d, "mom": mom}


def lsq(X, gidx, yw, drop=None):
    """score_g = |M^-1 d|^2 / s in longdouble with the bound at c = 1 and cond_2(M).  drop: {group: column offsets left out
    of the solve} (the later copy of an exact duplicate); s stays the group's width."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    gidx, sizes = layout(gidx, p)
    Xl, ywl = ld(X), ld(yw)
    gram1 = xprec.GRAM_FACTOR * np.sqrt(float(n)) * U
    ywn = float(np.sqrt(ywl @ ywl))
    out, bound, conds = np.zeros(len(sizes), dtype=LD), np.zeros(len(sizes)), np.zeros(len(sizes))
    for g, (c0, s) in enumerate(zip(gidx, sizes)):
        keep = [u for u in range(s) if u not in (drop or {}).get(g, ())]
        Xg = Xl[:, c0:c0 + s][:, keep]
        if not (Xg * Xg).sum(axis=0).all():
            out[g], bound[g], conds[g] = np.inf, 0.0, 1.0  # an all-zero column
            continue
        M, d = Xg.T @ Xg, Xg.T @ ywl
        xn = np.sqrt(np.diag(M).astype(np.float64))
        E = gram1 * np.outer(xn, xn)
        e_d = gram1 * xn * ywn
        L = chol(M)
        z = bwd(L, fwd(L, d))
        Minv = np.abs(np.stack([bwd(L, fwd(L, e)) for e in np.eye(len(keep), dtype=LD)])).astype(np.float64)
        az = np.abs(z).astype(np.float64)
        conds[g] = xprec.cond(M)
        zz = float(z @ z)
        out[g] = (z @ z) / LD(s)
        bound[g] = (2 * az @ Minv @ (e_d + E @ az) + 2 * len(keep) * U * conds[g] * zz) / s + 4 * U * float(out[g])
    return {"score": out, "bound": bound, "cond": conds}


# ---- fp64 NumPy evaluating the kernels' formulas (the CPU stand-in, never the kernels) ----------------------------------------
def moments_fp64(case, cshift=0, drop_rows=None, zero_tile=None, transpose_tile=None, panel_dcol=False):
    """mblk (list of blocks; None for the groups before column cshift) and dcol in fp64.  drop_rows (row indices left out),
    zero_tile / transpose_tile ((group, tu, tv): that 8 x 8 tile of the block and its mirror image left at zero / filled
    with X_v'X_u where X_u'X_v belongs) and panel_dcol (dcol written at the panel's column index instead of the global one)
    are the stand-in defects of tests/test_group_reference.py."""
    X = np.asarray(case["X"], dtype=np.float64)
    n, p = X.shape
    gidx, sizes = layout(case["gidx"], p)
    keep = np.ones(n, dtype=bool)
    if drop_rows is not None:
        keep[np.asarray(drop_rows, dtype=int)] = False
    w1 = np.ones(n) if case["w1"] is None else np.asarray(case["w1"], dtype=np.float64)
    dcol = np.zeros(p) if case.get("dcol") is None else np.array(case["dcol"], dtype=np.float64)
    blocks = []
    for g, (c0, s) in enumerate(zip(gidx, sizes)):
        if c0 < cshift:
            blocks.append(None)
            continue
        Xg = X[keep, c0:c0 + s]
        M = Xg.T @ (w1[keep, None] * Xg)
        M = np.tril(M) + np.tril(M, -1).T  # (one triangle computed, mirrored: as the kernels write it)
        for tile, how in ((zero_tile, "zero"), (transpose_tile, "transpose")):
            if tile is not None and tile[0] == g:
                u, v = slice(tile[1] * TILE, tile[1] * TILE + TILE), slice(tile[2] * TILE, tile[2] * TILE + TILE)
                blk = np.zeros_like(M[u, v]) if how == "zero" else M[u, v].T.copy()  # (transposed: full tiles only)
                M[u, v], M[v, u] = blk, blk.T
        blocks.append(M)
        if case["w2"] is not None:
            at = c0 - cshift if panel_dcol else c0
            dcol[at:at + s] = Xg.T @ np.asarray(case["w2"], dtype=np.float64)[keep]
    return blocks, dcol


def scores_fp64(case, blocks, dcol, form, nt_in_d=True, ridge="diagonal", divide_by=None, eig_from=None):
    """bd of every group in fp64 from fp64 moments; form "eigh" (the sqrtm form) or "chol".  nt_in_d (False: the division
    of d by n_t left out), ridge ("all": 2 lam added to every entry, "none": left out), divide_by (a number instead of s)
    and eig_from ({group: the group whose eigenvectors it is fed}, form "eigh") are the stand-in defects."""
    p = np.shape(case["X"])[1]
    gidx, sizes = layout(case["gidx"], p)
    lam, beta = float(case["lam"]), np.asarray(case["beta"], dtype=np.float64)
    if case["lm"]:
        d0 = np.atleast_2d(case["part"]).sum(axis=0)
        if nt_in_d:
            d0 = d0 / case["n_t"]
    else:
        d0 = dcol
    d = d0 - 2 * lam * beta
    Ms = []
    for g, s in enumerate(sizes):
        M = blocks[g] / case["n_t"] if case["lm"] else blocks[g].copy()
        Ms.append(M + 2 * lam * {"diagonal": np.eye(s), "all": np.ones((s, s)), "none": np.zeros((s, s))}[ridge])
    out = np.zeros(len(sizes))
    for g, (c0, s) in enumerate(zip(gidx, sizes)):
        b, dg = beta[c0:c0 + s], d[c0:c0 + s]
        with np.errstate(all="ignore"):
            if form == "eigh":
                lv, V = np.linalg.eigh(Ms[g])
                if eig_from is not None and g in eig_from:
                    V = np.linalg.eigh(Ms[eig_from[g]])[1]
                sq = np.sqrt(lv)
                t = V @ (sq * (V.T @ b) + (V.T @ dg) / sq)
            else:
                L = np.linalg.cholesky(Ms[g])
                t = L.T @ b + np.linalg.solve(L, dg)
        out[g] = (t @ t) / (s if divide_by is None else divide_by)
    return out


def lsq_fp64(X, gidx, yw, form, drop=None):
    """form "chol" (Cholesky and two substitutions) or "solve" (LU); drop as lsq()."""
    X = np.asarray(X, dtype=np.float64)
    gidx, sizes = layout(gidx, X.shape[1])
    out = np.zeros(len(sizes))
    for g, (c0, s) in enumerate(zip(gidx, sizes)):
        Xg = X[:, c0:c0 + s][:, [u for u in range(s) if u not in (drop or {}).get(g, ())]]
        if not (Xg * Xg).sum(axis=0).all():
            out[g] = np.inf
            continue
        M, d = Xg.T @ Xg, Xg.T @ np.asarray(yw, dtype=np.float64)
        if form == "chol":
            L = np.linalg.cholesky(M)
            z = np.linalg.solve(L.T, np.linalg.solve(L, d))
        else:
            z = np.linalg.solve(M, d)
        out[g] = (z @ z) / s
    return out


# ---- the assertion helpers: each returns the fraction of its bound that was used ----------------------------------------------
def assert_moments_close(blocks, mom, what, only=None):
    """Every entry of every block (of the groups in `only`, all without) inside xprec's Gram bound, and exactly symmetric."""
    worst = 0.0
    for g, (c0, s) in enumerate(zip(mom["gidx"], mom["sizes"])):
        if only is not None and g not in only:
            continue
        B = np.asarray(blocks[g], dtype=np.float64)
        assert B.shape == (s, s) and np.isfinite(B).all(), (what, g, B.shape)
        assert np.array_equal(B, B.T), (what, "block %d is not symmetric" % g)
        nr = mom["norms"][c0:c0 + s]
        worst = max(worst, xprec.assert_gram_close(B, mom["mblk"][g], nr, nr, mom["n"], "%s group %d" % (what, g)))
    print("%s: moments at %.3f of the Gram bound" % (what, worst))
    return worst


def assert_dcol_close(dcol, case, mom, what, lo=0):
    """X'w2 inside its bound from column lo on; without w2, dcol is bitwise what it was."""
    dcol = np.asarray(dcol, dtype=np.float64)
    if case["w2"] is None:
        assert np.array_equal(dcol, np.asarray(case["dcol"], dtype=np.float64)), (what, "dcol was written without w2")
        return 0.0
    f = _frac(np.abs(ld(dcol) - mom["dcol"])[lo:], mom["e_dcol"][lo:])
    f = np.where(np.isfinite(dcol[lo:]), f, np.inf)
    j = int(np.argmax(f))
    print("%s: dcol at %.3f of its bound (column %d)" % (what, f[j], lo + j))
    assert f[j] <= 1.0, (what, lo + j, dcol[lo + j], float(mom["dcol"][lo + j]), f[j])
    return float(f[j])


def score_units(bd, sref, skip=None, lo=0):
    """max_g |bd_g - bd*_g| / (the bound at c = 1) over the groups from lo on that `skip` (flags) leaves, and the group."""
    bd = np.asarray(bd, dtype=np.float64)
    use = np.arange(bd.size) >= lo
    if skip is not None:
        use &= ~np.asarray(skip).astype(bool)
    bd = np.where(use, bd, sref["bd"].astype(np.float64))
    f = _frac(np.abs(ld(bd) - sref["bd"]), sref["bound"])
    f = np.where(use, np.where(np.isfinite(bd), f, np.inf), 0.0)
    g = int(np.argmax(f))
    return float(f[g]), g, use


def assert_scores_close(bd, sref, what, skip=None, lo=0):
    r, g, use = score_units(bd, sref, skip, lo)
    cmax = float(sref["cond"][use].max()) if use.any() else 1.0
    assert cmax <= COND_LIMIT, (what, "a group is too ill-conditioned for its bound to test the score", cmax)
    print("%s: bd at %.3f of its bound (c = %.3f of %g, group %d, largest cond %.3g)" % (what, r / SCORE_C, r, SCORE_C, g, cmax))
    assert r <= SCORE_C, (what, g, float(np.asarray(bd)[g]), float(sref["bd"][g]), r, SCORE_C)
    return r / SCORE_C


def lsq_units(score, ref):
    score = np.asarray(score, dtype=np.float64)
    fin = np.isfinite(ref["score"].astype(np.float64))
    f = np.zeros(score.size)
    f[fin] = _frac(np.abs(ld(score[fin]) - ref["score"][fin]), ref["bound"][fin])
    f[fin] = np.where(np.isfinite(score[fin]), f[fin], np.inf)
    f[~fin] = np.where(score[~fin] == np.inf, 0.0, np.inf)  # +inf exactly, never NaN
    g = int(np.argmax(f))
    return float(f[g]), g


def assert_lsq_close(score, ref, what):
    r, g = lsq_units(score, ref)
    assert float(ref["cond"].max()) <= COND_LIMIT, (what, float(ref["cond"].max()))
    print("%s: lsq score at %.3f of its bound (c = %.3f of %g, group %d)" % (what, r / LSQ_C, r, LSQ_C, g))
    assert r <= LSQ_C, (what, g, float(np.asarray(score)[g]), float(ref["score"][g]), r, LSQ_C)
    return r / LSQ_C


# ---- seeded cases, one place for both files -----------------------------------------------------------------------------------
# widths of the groups of one call, by the moment template their widest group selects (k_group_moments<2|4|8|16>, and _big
# beside <16>): every compile-time width of k_group_score (1 .. 8), run-time widths 9 .. 16, and past GRP_MAX the tile grids of
# 17 (3 tile rows, 6 tiles, a 1-column last tile), 24 (3, exact), 25 (4 tile rows, 10 tiles, 1 column), 40 (5, 15 tiles, exact)
# and 29 (4 tile rows, a ragged last tile of 5 columns: the u0 + a < s / v0 + b < s guards with several live columns)
WIDTHS = {2: (1, 2, 2, 1, 2), 4: (3, 1, 4, 2, 3), 8: (5, 7, 8, 1, 6, 3, 2, 4), 16: (9, 16, 2, 12, 5, 10),
          40: (17, 3, 24, 1, 25, 8, 40, 16, 9, 29)}
ROWS = (1, 2, 255, 256, 257, 1000)
GROUP_COUNTS = (1, 63, 64, 65)
NOISES = (None, 1e-3, 1e-5)


def make_case(widths, n, q, noise=None, seed=0):
    """One call's inputs.  q picks the options so that every value of each meets every template and row count:
    w1 / w2 given or not, lam 0 or 0.05 (0.05 wherever n is below the widest group), beta zero or not, lm with n_t != n
    and nrb 1 or 3, always flags.  noise: the last column of every group of two or more = its first + noise x N(0, 1)."""
    widths = tuple(int(s) for s in widths)
    p, N = sum(widths), len(widths)
    rng = _rng(p, N, n, q, seed, 0 if noise is None else int(round(-np.log10(noise))))
    gidx = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(np.int32)
    X = rng.standard_normal((n, p))
    if noise is not None:
        for c0, s in zip(gidx, widths):
            if s >= 2:
                X[:, c0 + s - 1] = X[:, c0] + noise * rng.standard_normal(n)
    lm = q % 2 == 1
    lam = 0.05 if (q // 4) % 2 == 1 or n < max(widths) + 8 else 0.0
    has_w1, has_w2 = q % 3 != 0, (q % 4 < 2) and not lm
    beta = np.zeros(p)
    if q % 3 != 1:
        for g in range(0, N, 3):
            beta[gidx[g]:gidx[g] + widths[g]] = rng.uniform(0.2, 1.0, widths[g]) * rng.choice([-1.0, 1.0], widths[g])
    w1 = w2 = part = None
    n_t = 1.0
    if lm:  # w1 = the 0 / 1 mask of a row set, d from the score pass's partials
        if has_w1:
            w1 = (rng.uniform(size=n) >= 0.2).astype(np.float64)
            w1[[0, n - 1]] = 1.0
            if n > 2:
                w1[n - 2] = 1.0  # (the last row pair counts: a dropped pair shows)
            n_t = float(w1.sum()) if n > 2 else float(n + 1)
        else:
            n_t = float(n + 3)
        part = rng.standard_normal((1 if q % 4 == 1 else 3, p)) * n_t / 3.0
    else:
        if has_w1:
            w1 = glmref._weights(n, rng)
            w1[n - 1] = w1[n - 1] or 0.75
        if has_w2:
            w2 = rng.standard_normal(n)
    always = None
    if q % 5 in (0, 3) and N > 1:
        always = np.zeros(N, dtype=np.uint8)
        always[[1, N - 1]] = 1
        always[int(np.argmax(widths))] = 1  # (one flag on the widest group: both score kernels write it)
    return {"X": X, "gidx": gidx, "w1": w1, "w2": w2, "beta": beta, "lm": lm, "n_t": n_t, "lam": lam, "part": part,
            "always": always, "dcol": rng.standard_normal(p), "widths": widths}


def count_widths(N):
    """N groups cycling through the compile-time widths and 9 (run-time loop): the 64-thread blocks of k_group_score."""
    return tuple((1, 2, 3, 4, 5, 7, 8, 9)[g % 8] for g in range(N))


def all_score_cases():
    """name -> case over everything the GPU file runs through op_group_scores."""
    out = {}
    for k, smax in enumerate(sorted(WIDTHS)):
        for j, n in enumerate(ROWS):
            q = 2 * k + 5 * j
            out["t smax=%d n=%d q=%d" % (smax, n, q)] = make_case(WIDTHS[smax], n, q)
            out["t smax=%d n=%d q=%d" % (smax, n, q + 1)] = make_case(WIDTHS[smax], n, q + 1)
    for j, N in enumerate(GROUP_COUNTS):
        for q in (3 * j, 3 * j + 7):
            out["g N=%d q=%d" % (N, q)] = make_case(count_widths(N) if N > 1 else ((5,), (24,))[q % 2], 257, q, seed=1)
    for noise in NOISES[1:]:
        for smax in (4, 8, 16, 40):
            for q in (0, 1, 4):  # lam = 0 in q = 0, 1 (lm = 0 / 1), 0.05 in q = 4
                out["c smax=%d noise=%g q=%d" % (smax, noise, q)] = make_case(WIDTHS[smax], 257, q, noise=noise, seed=2)
    return out


def panel_case():
    """A design with wide and narrow groups whose groups 3 .. are also run as a panel (cshift)."""
    return make_case(WIDTHS[40], 257, 0, seed=3)


def panel_of(case, g0=3):
    """The same call on the columns from group g0 on: (case with X cut, cshift)."""
    cs = int(case["gidx"][g0])
    cut = dict(case)
    cut["X"] = np.ascontiguousarray(case["X"][:, cs:])
    return cut, cs


LSQ_WIDTHS = (1, 5, 17, 40, 5, 17, 3, 2)
LSQ_DUP = {4: (1, 3), 5: (4, 16)}  # group -> (column, its later copy)
LSQ_ZERO = (6, 1)                  # group, its all-zero column
LSQ_ROWS = (257, 1000)


def lsq_case(n):
    """(X, gidx, yw, drop): full-rank groups of 1, 5, 17 and 40 columns, two groups with an exact duplicate inside, one with
    an all-zero column, one more full-rank group behind them."""
    rng = _rng(n, 4242)
    p = sum(LSQ_WIDTHS)
    gidx = np.concatenate([[0], np.cumsum(LSQ_WIDTHS)[:-1]]).astype(np.int32)
    X = rng.standard_normal((n, p))
    for g, (a, b) in LSQ_DUP.items():
        X[:, gidx[g] + b] = X[:, gidx[g] + a]
    X[:, gidx[LSQ_ZERO[0]] + LSQ_ZERO[1]] = 0.0
    yw = X[:, 0] - 0.5 * X[:, 3] + 0.7 * X[:, 30] + rng.standard_normal(n)
    return X, gidx, yw, {g: (b,) for g, (a, b) in LSQ_DUP.items()}


def lsq_short_case():
    """(X, gidx, yw, drop) with more columns than rows: n = 3, groups of 5, 2 and 3 columns.  The last two columns of the
    first group depend on its first three and are dropped; the others have full rank."""
    rng = _rng(3, 4243)
    X = rng.standard_normal((3, 10))
    return X, np.array([0, 5, 7], dtype=np.int32), rng.standard_normal(3), {0: (3, 4)}
