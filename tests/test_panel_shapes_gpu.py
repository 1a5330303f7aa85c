"""GPU: the Gram panel pass (k_cov_panel_dp) at small shapes, every launch kind it has.

The kernel walks a row slab in 32-row chunks through two LDS tiles, its one barrier per chunk between the chunk's two row
steps and the operands of every step read one step ahead -- those of a chunk's first step during the chunk before, out
of the tile that chunk stored -- and a two-group launch splits the right-hand-side tiles between the two halves of the
workgroup, two streamed tiles per wave.

Shapes.  Rows 20, 33, 65, 97, 130, 600, 1100 and columns 96, 130, 257 are the list of the change's issue.  What they
exercise THROUGH A SESSION is less than the row counts suggest: a session pads its rows to a multiple of 128 (the padding
is zero) and cuts slabs in multiples of 64 rows, and the kernel counts chunks over the padded rows.  So n = 20 .. 97 run
one slab of 4 chunks, n = 130 one of 8, n = 600 two slabs (320 + 320 padded rows), n = 1100 four; every slab has an even
chunk count and no chunk is partial.  The loop's exit on an odd count and a slab shorter than the three-chunk prologue
cannot be reached through the library (as before this kernel's restructuring) and are NOT tested here.  What the rows
do vary is the share of zero padding in the last chunks and the number of slabs the reduce kernel adds.  The columns:
96 is one workgroup; 130 two, the last with 2 columns and nothing to write for its second half; 257 three.

Launch kinds.
  * one-group and two-group launches of full lists (32 and 64 columns) through the prefill route, bit for bit the same
    columns, each against np.longdouble arithmetic on the library's own normalised columns under the bound of
    tests/test_lm_precision_gpu.py::test_gram_columns_of_the_prefill_route (xprec.assert_gram_close);
  * the prefill route lists whole groups of 32 columns and never launches beyond its list, so the remaining kinds are
    driven through fits whose INITIAL model has 40 columns (the fill at the start of a fit lists the model's missing
    columns without speculative ones and launches (40 + 31) / 32 = 2 groups, bessx_fit.cpp "cov begin"):
      - a 40-column list: 64 entries, 24 of them -1, one two-group launch;
      - a two-group launch whose second group lies beyond the list: 32 of the 40 columns missing, a list of 32, and the
        device runs the one-group instance;
      - the masked instance of the two-group code: the 40-column list on a fold of a session with 3 CV folds whose row
        sets are filled one masked pass each (test hook cv_shared=0, as tests/test_cov_gpu.py does it).
    Each asserts from the session's counters that the launch it is about happened (groups formed on the device, launches
    by real width, columns cached) and compares the fit with NumPy's least squares on the same rows.
  * paths (sequential; golden section over 3 masked folds) at every shape against the oracle's trace: one-group fills of
    running paths."""
import numpy as np
import pytest

import xprec
from helpers import assert_same_trace, hooks
from oracle import port_ctypes as P
from bess_amd import synth

pytestmark = pytest.mark.gpu

ROWS = (20, 33, 65, 97, 130, 600, 1100)
COLUMNS = (96, 130, 257)
SHAPES = [(n, p) for n in ROWS for p in COLUMNS]
_cases = {}


def _case(gpu, n, p):
    """Design, weights, the 64 listed columns and their longdouble Gram columns: computed once per shape."""
    if (n, p) not in _cases:
        X, y = xprec.design_large_mean(n, p)
        w = xprec.weights(n)
        Xs = gpu.op_normalize(X, y, w, 1, True, True)[0]
        cols = ((np.arange(64) * 29 + 7) % p).astype(np.int32)
        assert np.unique(cols).size == 64
        want = xprec.gram_columns(Xs, None, cols)
        want.setflags(write=False)
        norms = np.sqrt((Xs * Xs).sum(axis=0))
        _cases[(n, p)] = (X, y, w, cols, want, norms)
    return _cases[(n, p)]


def _export(s, cols, passes, p):
    s.cov_prefill_begin(cols)
    for g0, ng in passes:
        s.cov_prefill_compute(g0, ng)
    got = s.cov_prefill_export(0, cols.size // 32).reshape(cols.size, p).T.copy()
    s.cov_prefill_end()
    return got


@pytest.mark.parametrize("n,p", SHAPES)
def test_gram_columns_of_one_and_two_group_launches(gpu, n, p):
    """Lists of 32 and of 64 columns; the 64 as two one-group launches and as one two-group launch."""
    X, y, w, cols, want, norms = _case(gpu, n, p)
    with gpu.Session(X, y, weight=w, score_mode=2) as s:
        one32 = _export(s, cols[:32], [(0, 1)], p)
        one64 = _export(s, cols, [(0, 1), (1, 1)], p)
        two64 = _export(s, cols, [(0, 2)], p)
    f = xprec.assert_gram_close(one64, want, norms[cols], norms, n, "Gram n=%d p=%d, one group per launch" % (n, p))
    print("n=%d p=%d: %.3f of the bound" % (n, p, f))
    assert np.array_equal(two64, one64), "a two-group launch differs from two one-group launches of the same columns"
    assert np.array_equal(one32, one64[:, :32]), "a list of 32 columns differs from the first group of a list of 64"
    sub = two64[cols, :]
    assert np.array_equal(sub, sub.T), "exported Gram columns are not bitwise symmetric"


def _levels(n):
    return max(3, min(12, n // 8))


@pytest.mark.parametrize("n,p", SHAPES)
def test_fills_of_a_path_and_of_masked_row_sets(gpu, monkeypatch, n, p):
    """The one-group fills of a path of up to 12 levels, unmasked and masked (3 CV folds, one masked pass per row set),
    against the oracle's trace."""
    X, y, _, _ = synth.make_lm(n, p, 3, seed=7 * n + p)
    smax = _levels(n)
    seq = np.arange(1, smax + 1)
    fold = synth.make_cv_folds(n, 3, seed=3)
    want = P.trace(X, y, ic_type=3, sequence=seq)
    want_cv = P.trace(X, y, ic_type=3, is_cv=True, K=3, cv_fold_id=fold, path_type=2, s_min=1, s_max=smax)
    # the criterion is n log(loss) + a penalty: the 1e-9 relative that assert_same_trace allows the loss is n 1e-9
    # absolute in a criterion value, whatever its size (the two terms cancel at some levels)
    ic_atol = 1e-9 * n
    hooks(monkeypatch, cv_shared="0")
    with gpu.Session(X, y, score_mode=2) as s:
        s.trace_enable(True)
        out = s.sequential_path(seq, ic_type=3)
        assert_same_trace(out["trace"], want, what="n=%d p=%d sequential" % (n, p), ic_atol=ic_atol)
        assert s.counters()["passes_over_X"] > 0
        s.set_cv(3, fold)
        cv = s.gs_path(1, smax, ic_type=3, is_cv=True)
        assert_same_trace(cv["trace"], want_cv, what="n=%d p=%d masked row sets" % (n, p), ic_atol=ic_atol)


# ---- launches a full list cannot make: 40-column list, second group beyond the list, masked pair --------------------------
PAIR_SHAPES = [(n, p) for n in (130, 600, 1100) for p in COLUMNS]  # (a model of 40 columns needs more than 40 training rows)
K40 = 40
_strong = {}


def _strong_case(n, p):
    """A design whose 40 true columns are unmistakable, in the session's normalised scale (centred, |x_j| = sqrt(n))."""
    if (n, p) not in _strong:
        X, y, S, _ = synth.make_lm(n, p, K40, seed=11 * n + p)
        S = np.sort(np.asarray(S)).astype(np.int32)
        assert S.size == K40
        Xc = X - X.mean(axis=0)
        Xn = np.sqrt(float(n)) * Xc / np.sqrt((Xc * Xc).sum(axis=0))
        _strong[(n, p)] = (X, y, S, Xn, y - y.mean())
    return _strong[(n, p)]


def _ls(Xn, yn, rows, S):
    return np.linalg.lstsq(Xn[rows][:, S], yn[rows], rcond=None)[0]


def _delta(after, before):
    return {k: after[k] - before[k] for k in ("passes_over_X", "panel_launches_one_group", "panel_launches_two_groups")}


def _assert_fit(r, S, b, what):
    o = np.argsort(r["support"])
    assert np.array_equal(r["support"][o], S), what + ": support"
    np.testing.assert_allclose(r["beta"][o], b, rtol=1e-8, atol=1e-10 * np.max(np.abs(b)), err_msg=what)


@pytest.mark.parametrize("n,p", PAIR_SHAPES)
def test_list_of_40_columns_is_one_padded_two_group_launch(gpu, n, p):
    X, y, S, Xn, yn = _strong_case(n, p)
    b = _ls(Xn, yn, np.ones(n, bool), S)
    with gpu.Session(X, y, score_mode=2) as s:
        s.enable_kernel_timing(True)
        c0 = s.counters()
        r = s.fit(K40, 0.0, -1, init_idx=S, init_val=b)
        d = _delta(s.counters(), c0)
        cached = int((s.cov_state()[1] >= 0).sum())
    print("n=%d p=%d: %s, %d columns cached, %d iterations" % (n, p, d, cached, r["iters"]))
    _assert_fit(r, S, b, "n=%d p=%d" % (n, p))
    # 40 columns cached by 2 groups in ONE launch of real width 2: a list of 64 entries, 24 of them padding
    assert cached == K40 and d == {"passes_over_X": 2, "panel_launches_one_group": 0, "panel_launches_two_groups": 1}, (d, cached)


@pytest.mark.parametrize("n,p", PAIR_SHAPES)
def test_second_group_beyond_the_list_runs_the_one_group_instance(gpu, n, p):
    X, y, S, Xn, yn = _strong_case(n, p)
    b = _ls(Xn, yn, np.ones(n, bool), S)
    others = np.setdiff1d(np.arange(p, dtype=np.int32), S)
    first = np.concatenate([S[:8], others[:56]]).astype(np.int32)  # 64 cached columns, 8 of them the model's
    with gpu.Session(X, y, score_mode=2) as s:
        s.enable_kernel_timing(True)
        s.cov_prefill_begin(first)
        s.cov_prefill_compute(0, 2)
        s.cov_prefill_end()
        assert int((s.cov_state()[1] >= 0).sum()) == 64
        c0 = s.counters()
        r = s.fit(K40, 0.0, -1, init_idx=S, init_val=b)
        d = _delta(s.counters(), c0)
        cached = int((s.cov_state()[1] >= 0).sum())
    print("n=%d p=%d: %s, %d columns cached, %d iterations" % (n, p, d, cached, r["iters"]))
    _assert_fit(r, S, b, "n=%d p=%d" % (n, p))
    # the fit's start launches 2 groups for its 40 columns; 32 are missing: a list of 32, ONE group formed, real width 1
    assert cached == 96 and d == {"passes_over_X": 1, "panel_launches_one_group": 1, "panel_launches_two_groups": 0}, (d, cached)


@pytest.mark.parametrize("n,p", PAIR_SHAPES)
def test_masked_two_group_launch_on_a_cv_fold(gpu, monkeypatch, n, p):
    X, y, S, Xn, yn = _strong_case(n, p)
    fold = synth.make_cv_folds(n, 3, seed=3)
    train = fold != 1
    b = _ls(Xn, yn, train, S)
    hooks(monkeypatch, cv_shared="0")
    with gpu.Session(X, y, score_mode=2) as s:
        s.set_cv(3, fold)
        s.enable_kernel_timing(True)
        c0 = s.counters()
        r = s.fit(K40, 0.0, 1, init_idx=S, init_val=b)
        d = _delta(s.counters(), c0)
    print("n=%d p=%d: %s, %d iterations" % (n, p, d, r["iters"]))
    _assert_fit(r, S, b, "n=%d p=%d fold 1" % (n, p))
    assert d == {"passes_over_X": 2, "panel_launches_one_group": 0, "panel_launches_two_groups": 1}, d
