"""What tests/test_cv_gram_gpu.py and tests/test_cv_gram_reference.py share: the cases, the folds, a pure-Python replica
of the rule by which bessx_session_set_cv lays out the fold-major copy of X (or refuses it), and a CPU stand-in that sums
fp64 slab partials in the device's order.  No GPU, no library call.

The rule (bessx_session.cpp, set_cv).  With nmax the largest fold's row count and K folds:
    cvp_nsl = max(1, (nmax + 1023) // 2048)                   slabs per fold
    cvp_rps = ceil(ceil(nmax / cvp_nsl) / 64) * 64            rows per slab
    copy    = K * cvp_nsl * cvp_rps rows                      every fold padded with zero rows to cvp_nsl whole slabs
and the copy is refused (the folds' row sets are then filled one masked pass each) when 2 * copy > 3 * ld, ld = the
session's own padded row count: n rounded up to 128 * U, U = 8, 4, 2, 1 for n >= 4096, 2048, 1024, below.
Row set r >= 1 (training rows of fold r - 1) sums every slab but [(r - 1) * cvp_nsl, r * cvp_nsl); row set 0 all."""
import numpy as np

from bess_amd import synth

K40 = 40  # columns of a fit's initial model: its start-of-fit fill lists (40 + 31) // 32 = 2 groups


def session_rows(n):
    u = 8 if n >= 4096 else (4 if n >= 2048 else (2 if n >= 1024 else 1))
    rb = 128 * u
    return (n + rb - 1) // rb * rb


def fill_geometry(n, sizes):
    """What Session.cv_fill_geometry() must answer for folds of these sizes on n rows."""
    K, nmax = len(sizes), max(sizes)
    nsl = max(1, (nmax + 1023) // 2048)
    rps = ((nmax + nsl - 1) // nsl + 63) // 64 * 64
    rows = K * nsl * rps
    if 2 * rows > 3 * session_rows(n):
        return {"shared": False, "cvp_nsl": 0, "cvp_rps": 0, "copy_rows": 0}
    return {"shared": True, "cvp_nsl": nsl, "cvp_rps": rps, "copy_rows": rows}


def folds_of_sizes(n, sizes, seed=23):
    """Fold id per row for folds of exactly these sizes, the rows of every fold scattered over the design."""
    assert sum(sizes) == n
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(n)
    fold = np.empty(n, dtype=np.int32)
    fold[perm] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    return fold


def listed_columns(p):
    """The panel test's column list (tests/test_panel_shapes_gpu.py), carried on to 72: the first fit's 40 columns and a
    second model that shares 8 of them, so that its fill lists 32 -- one group."""
    cols = ((np.arange(72) * 29 + 7) % p).astype(np.int32)
    assert np.unique(cols).size == 72
    return np.sort(cols[:K40]), np.sort(cols[32:72])


class Case:
    """name: what the case reaches.  sizes: fold sizes (None: near-equal folds of synth.make_cv_folds).  want: the
    geometry the issue states for the case, where it states one; route: "sets" (shared fills, one reduce for all row
    sets), "per-set" (shared fills, K + 1 > 9: one reduce per row set), "refused" (the rule refuses the copy: masked
    fills), "hook" (masked fills by the test hook cv_shared=0)."""

    def __init__(self, name, route, n, p, K, sizes=None, want=None):
        self.name, self.route, self.n, self.p, self.K, self.sizes, self.want = name, route, n, p, K, sizes, want

    @property
    def id(self):
        return "%s-n%d-p%d-K%d" % (self.name, self.n, self.p, self.K)

    def fold(self):
        if self.sizes is None:
            return synth.make_cv_folds(self.n, self.K, seed=3)
        return folds_of_sizes(self.n, self.sizes)

    def fold_sizes(self):
        return [int(v) for v in np.bincount(self.fold(), minlength=self.K)]

    def geometry(self):
        if self.route == "hook":
            return {"shared": False, "cvp_nsl": 0, "cvp_rps": 0, "copy_rows": 0}
        return fill_geometry(self.n, self.fold_sizes())


def _near_equal():
    """K = 2, 3, 4, 8 at n in {130, 600, 1100}, p in {96, 130, 257}, near-equal folds.  The route follows from the rule:
    8 folds of 16-18 rows (n = 130) and of 75 rows (n = 600) pad to 8 slabs of 64 and of 128 rows, more than 1.5 times
    the session's 256 and 640 rows, and the copy is refused there -- those cases hold the masked fills to the bound."""
    out = []
    for K in (2, 3, 4, 8):
        for n in (130, 600, 1100):
            for p in (96, 130, 257):
                c = Case("near-equal", "sets", n, p, K)
                if not c.geometry()["shared"]:
                    c.name, c.route = "near-equal-refused", "refused"
                out.append(c)
    return out


NEAR_EQUAL = _near_equal()
# K + 1 > 9 row sets: one k_cov_reduce + k_cov_compact per row set.  K = 9 and 10 at n = 600 are the issue's; 9 folds of
# 66-72 rows pad to slabs of 128 rows and the rule refuses that copy (1152 rows against 1.5 x 640), so n = 576 -- 9 folds of
# exactly 64 rows -- is added to reach the per-row-set reduce at its threshold K + 1 = 10.
PER_SET = [Case("per-set-reduce", "refused", 600, 130, 9), Case("per-set-reduce", "per-set", 600, 130, 10),
           Case("per-set-reduce", "per-set", 576, 130, 9)]
UNEQUAL = [
    Case("every-fold-under-one-slab", "sets", 130, 130, 3, (60, 40, 30), {"shared": True, "cvp_nsl": 1, "cvp_rps": 64}),
    Case("one-row-over-a-slab", "sets", 193, 130, 3, (65, 64, 64), {"shared": True, "cvp_nsl": 1, "cvp_rps": 128}),
    Case("unequal", "sets", 600, 130, 3, (250, 200, 150), {"shared": True, "cvp_nsl": 1, "cvp_rps": 256}),
]
MULTI_SLAB = [
    Case("two-slabs-per-fold", "sets", 6145, 96, 2, (3073, 3072), {"shared": True, "cvp_nsl": 2}),
    Case("three-slabs-per-fold", "sets", 10241, 96, 2, (5121, 5120), {"shared": True, "cvp_nsl": 3}),
    Case("two-slabs-middle-fold", "sets", 9217, 96, 3, (3073, 3072, 3072), {"shared": True, "cvp_nsl": 2}),
]
REFUSED = [Case("copy-refused", "refused", 600, 130, 3, (500, 50, 50), {"shared": False})]
HOOK = [Case("masked-by-hook", "hook", n, p, 3) for n in (130, 600, 1100) for p in (96, 257)]
SHARED_CASES = NEAR_EQUAL + PER_SET + UNEQUAL + MULTI_SLAB + REFUSED


def masks(fold, K):
    """Row set r -> boolean mask of its rows: 0 all rows, r >= 1 the training rows of fold r - 1."""
    fold = np.asarray(fold)
    return [np.ones(fold.size, dtype=bool)] + [fold != k for k in range(K)]


def gram_in_device_order(Xs, fold, K, nsl, rps, r, cols, skip=None):
    """fp64 stand-in for the shared fills of row set r: the fold-major copy (fold k's rows ascending, then zero rows up to
    nsl slabs of rps rows), one fp64 partial per slab, the partials summed slab after slab without the slabs of `skip`
    (default: what the library leaves out, [(r - 1) * nsl, r * nsl), nothing for r = 0)."""
    Xs = np.asarray(Xs, dtype=np.float64)
    p = Xs.shape[1]
    seg = nsl * rps
    Xp = np.zeros((K * seg, p))
    for k in range(K):
        rows = np.nonzero(np.asarray(fold) == k)[0]
        Xp[k * seg:k * seg + rows.size] = Xs[rows]
    if skip is None:
        skip = (0, 0) if r == 0 else ((r - 1) * nsl, r * nsl)
    G = np.zeros((p, len(cols)))
    for sl in range(K * nsl):
        if skip[0] <= sl < skip[1]:
            continue
        blk = Xp[sl * rps:(sl + 1) * rps]
        G = G + blk.T @ blk[:, cols]
    return G
