"""GPU: the group-selection kernels, called alone through the C ABI (bessx_op_group_scores: k_group_moments<2|4|8|16>,
k_group_moments_big, k_group_score in eig_mode 0, 1 and 2, k_group_score_big; bessx_op_group_lsq: the moments with yw, then
k_group_lsq_score), against the longdouble reference of tests/groupref.py.  The bounds live in groupref.assert_*;
tests/test_group_reference.py shows on the CPU that fp64 NumPy sits inside them (that is where their constants come from),
that every helper fails on a result wrong at 1e-9, and that stand-ins of the defects this file exists for -- the last two
rows dropped from a moment, a tile of a wide block left at zero or transposed, the n_t division left out of d, the ridge off
the diagonal or left out, the score divided by GRP_MAX, another group's eigenvectors in eig_mode 2, dcol indexed by the panel
column under cshift -- fail.

(a) every moment template with every row count of groupref.ROWS (1, 2, 255, 256, 257, 1000: the 256-stride loop, the block
sum, n below the group width with lam > 0), widths 1 .. 8 (compile-time), 9 .. 16 (run-time loops) and 17, 24, 25, 40 (tile
grid) in mixed calls; w1 / w2 given or not (dcol bitwise untouched without w2), lam 0 and 0.05, beta zero and not, lm with
n_t != n and one or three row blocks, always flags (exactly DBL_MAX); (b) N = 1, 63, 64, 65 groups; (c) one column of every
group = another + 1e-3 / 1e-5 noise, under the bound that carries cond(M_g) (every case asserts cond <= groupref.COND_LIMIT);
(d) a cshift panel against the unshifted call, bitwise; (e) k_group_lsq_score on full-rank groups, exact duplicates and an
all-zero column.  In every call: mblk exactly symmetric, eig_mode 1 and 2 bitwise eig_mode 0, the call twice bitwise the same.

Not covered here: launch_cox_group_moments as a whole (its suffix-sum inputs need the Cox state; only its two calls of
launch_group_moments, with and without cshift, are), the ctrl gating of the score kernels (ctrl is null here), the
k_screen_*_group kernels.

Measured on an MI355X on 2026-10-19, on top of commit af913ce (every test prints the fraction of each bound it uses, -s shows
them), BEFORE the group of 29 columns joined the wide set and with the lsq figure restated for LSQ_C = 1 / 32: the file's 47
tests pass in 9.5 s (tests/test_glm_ops_gpu.py: 32 tests in 5.6 s), the slowest case 0.7 s.  Largest fraction of each bound
used: moments 0.051 and dcol 0.031 (both at n = 1, beside the wide groups), bd 0.054 (a group of one column at n = 1, lm;
0.107 of the expression at c = 1, where fp64 NumPy needs 0.274), lsq 0.26 (n = 3: 0.008 of the expression at c = 1, where
fp64 NumPy needs 0.0052; the other lsq cases 0.03).  eig_mode 1 and 2, the repeated calls and the cshift panel were bitwise
equal throughout.  No kernel had to change.  A build with one tile of k_group_moments_big reading the wrong operand and
eig_mode 2 loading the neighbouring group's eigenvectors failed 45 of the tests.  The bounds do not depend on these figures:
their constants come from fp64 NumPy on the CPU (groupref.*_NUMPY_MAX), the rest is derived."""
import numpy as np
import pytest

import groupref as R
import xprec

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not xprec.EXTENDED, reason="np.longdouble is not the x86 extended format")]

WORST = {}
_CASES = {}


def _cases():
    if not _CASES:
        _CASES.update(R.all_score_cases())
    return _CASES


def _note(**fracs):
    for k, v in fracs.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    print("largest fractions so far: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def _call(gpu, case, cshift=0, p=None):
    """op_group_scores twice: bitwise the same."""
    kw = dict(w1=case["w1"], w2=case["w2"], lm=case["lm"], n_t=case["n_t"], lam=case["lam"], always=case["always"],
              part=case["part"], dcol=case["dcol"], cshift=cshift, p=p)
    got = gpu.op_group_scores(case["X"], case["gidx"], case["beta"], **kw)
    again = gpu.op_group_scores(case["X"], case["gidx"], case["beta"], **kw)
    for k in ("mblk_flat", "dcol", "bd"):
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    return got


def _check(gpu, name, case):
    got = _call(gpu, case)
    mom = R.moments(case)
    sref = R.scores(case, mom)
    f = {"moments": R.assert_moments_close(got["mblk"], mom, name), "dcol": R.assert_dcol_close(got["dcol"], case, mom, name)}
    flags = None if case["always"] is None else case["always"].astype(bool)
    f["bd"] = R.assert_scores_close(got["bd"][0], sref, name, skip=flags)
    if flags is not None:
        assert flags.any() and (got["bd"][:, flags] == R.DBL_MAX).all(), (name, got["bd"][:, flags])
    # the stored decomposition: the same arithmetic, stored and loaded -- bit-identical scores (k_group_score's comment)
    assert np.array_equal(got["bd"][1], got["bd"][0]), (name, "eig_mode 1", np.nonzero(got["bd"][1] != got["bd"][0])[0])
    assert np.array_equal(got["bd"][2], got["bd"][0]), (name, "eig_mode 2", np.nonzero(got["bd"][2] != got["bd"][0])[0])
    _note(**f)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smax", sorted(R.WIDTHS))
@pytest.mark.parametrize("n", R.ROWS)
def test_moments_and_scores_at_every_template_and_row_count(gpu, smax, n):
    mine = {k: c for k, c in _cases().items() if k.startswith("t smax=%d n=%d " % (smax, n))}
    assert len(mine) == 2
    for name, case in mine.items():
        _check(gpu, name, case)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.GROUP_COUNTS)
def test_group_counts_around_the_64_thread_blocks(gpu, N):
    mine = {k: c for k, c in _cases().items() if k.startswith("g N=%d " % N)}
    assert len(mine) == 2 and all(len(c["widths"]) == N for c in mine.values())
    for name, case in mine.items():
        _check(gpu, name, case)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smax", (4, 8, 16, 40))
@pytest.mark.parametrize("noise", R.NOISES[1:])
def test_nearly_collinear_columns_under_the_bound_that_carries_the_condition_number(gpu, smax, noise):
    mine = {k: c for k, c in _cases().items() if k.startswith("c smax=%d noise=%g " % (smax, noise))}
    assert len(mine) == 3
    for name, case in mine.items():
        _check(gpu, name, case)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
def test_a_cshift_panel_gives_bitwise_the_blocks_of_the_unshifted_call(gpu):
    case = R.panel_case()
    g0 = 3
    panel, cs = R.panel_of(case, g0)
    p = case["X"].shape[1]
    whole, part = _call(gpu, case), _call(gpu, panel, cshift=cs, p=p)
    mom = R.moments(case)
    flags = None if case["always"] is None else case["always"].astype(bool)
    _note(moments=R.assert_moments_close(whole["mblk"], mom, "panel case"),
          dcol=R.assert_dcol_close(whole["dcol"], case, mom, "panel case"),
          bd=R.assert_scores_close(whole["bd"][0], R.scores(case, mom), "panel case", skip=flags))
    for g in range(g0, len(case["widths"])):
        assert np.array_equal(part["mblk"][g], whole["mblk"][g]), g
    for g in range(g0):
        assert not part["mblk"][g].any(), g  # (not launched)
    assert np.array_equal(part["dcol"][cs:], whole["dcol"][cs:])
    assert np.array_equal(part["dcol"][:cs], case["dcol"][:cs])  # global indexing: nothing before the panel is written
    assert np.array_equal(part["bd"][:, g0:], whole["bd"][:, g0:])


# ---- (e) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.LSQ_ROWS)
def test_lsq_score_full_rank_duplicate_and_zero_columns(gpu, n):
    X, gidx, yw, drop = R.lsq_case(n)
    got = gpu.op_group_lsq(X, gidx, yw)
    assert np.array_equal(got, gpu.op_group_lsq(X, gidx, yw), equal_nan=True)
    ref = R.lsq(X, gidx, yw, drop)  # (the later copy of each duplicate dropped, s kept)
    assert got[R.LSQ_ZERO[0]] == np.inf and not np.isnan(got).any(), got
    _note(lsq=R.assert_lsq_close(got, ref, "lsq n=%d" % n))
    flags = np.zeros(len(gidx), dtype=np.uint8)
    flags[[1, R.LSQ_ZERO[0]]] = 1
    flagged = gpu.op_group_lsq(X, gidx, yw, always=flags)
    assert (flagged[flags == 1] == R.DBL_MAX).all() and np.array_equal(flagged[flags == 0], got[flags == 0])


def test_lsq_score_with_more_columns_than_rows(gpu):
    """n = 3 under a group of 5: the columns that depend on the ones before them are dropped (k_group_lsq_score's comment)."""
    X, gidx, yw, drop = R.lsq_short_case()
    got = gpu.op_group_lsq(X, gidx, yw)
    assert np.array_equal(got, gpu.op_group_lsq(X, gidx, yw))
    _note(lsq=R.assert_lsq_close(got, R.lsq(X, gidx, yw, drop), "lsq n=3"))


def test_bad_arguments_are_refused(gpu):
    case = R.make_case((2, 3), 5, 0)
    with pytest.raises(gpu.BessxError):
        gpu.op_group_scores(case["X"], [0, 2], case["beta"], lm=True)  # lm without part
    with pytest.raises(gpu.BessxError):
        gpu.op_group_scores(case["X"][:, 1:], [0, 2], case["beta"], cshift=1, p=5)  # cshift inside a group
    with pytest.raises(gpu.BessxError):
        gpu.op_group_lsq(case["X"], [0, 3, 3], np.ones(5))  # an empty group
