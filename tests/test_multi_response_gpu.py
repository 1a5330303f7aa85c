"""Many responses against one design (bessx_session_set_responses / bessx_session_sequential_path_multi, bess_amd/csrc/
bessx_multi.cpp): the responses' sequential paths as chains of ONE merged run on one Gram column cache.  Every response's
result must be the one a session created with that column as its y returns: supports and PDAS iterations bit-exact,
criteria and coefficients to the chunk chains' standard."""
import os

import numpy as np
import pytest

import helpers
from bess_amd import linear, synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "fullsize_lm.npz")


def _same(a, b, what):
    np.testing.assert_array_equal(a["cand_T0"], b["cand_T0"], err_msg=what)
    np.testing.assert_array_equal(a["cand_support"], b["cand_support"], err_msg=what + " supports")
    np.testing.assert_array_equal(a["cand_iters"], b["cand_iters"], err_msg=what + " PDAS iterations")
    np.testing.assert_allclose(a["cand_train_loss"], b["cand_train_loss"], rtol=1e-11, atol=1e-300, err_msg=what)
    np.testing.assert_allclose(a["cand_ic"], b["cand_ic"], rtol=1e-11, err_msg=what)
    np.testing.assert_allclose(a["cand_beta"], b["cand_beta"], rtol=1e-9, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(a["cand_coef0"], b["cand_coef0"], rtol=1e-9, atol=1e-12, err_msg=what)
    assert a["best_T0"] == b["best_T0"] and a["n_candidates"] == b["n_candidates"], what
    np.testing.assert_array_equal(np.nonzero(a["beta"])[0], np.nonzero(b["beta"])[0], err_msg=what + " best model")
    np.testing.assert_allclose(a["beta"], b["beta"], rtol=1e-9, atol=1e-12, err_msg=what)
    np.testing.assert_allclose([a["coef0"], a["train_loss"], a["ic"]], [b["coef0"], b["train_loss"], b["ic"]],
                               rtol=1e-9, atol=1e-12, err_msg=what)


def _singles(gpu, X, Y, seq, lam=(0.0,), ic_type=3, **kw):
    out = []
    for r in range(Y.shape[1]):
        with gpu.Session(X, Y[:, r], **kw) as s:
            out.append(s.sequential_path(seq, lam, ic_type=ic_type))
    return out


def _multi(gpu, X, Y, seq, lam=(0.0,), ic_type=3, **kw):
    with gpu.Session(X, Y[:, 0], **kw) as s:
        s.set_responses(Y)
        res = s.sequential_path_multi(seq, lam, ic_type=ic_type)
        return res, s.counters()


def _responses(X, R, seed):
    """Fresh signals on random supports, and permutations of the first one."""
    rng = np.random.default_rng(seed)
    n, p = X.shape
    Y = np.empty((n, R))
    for r in range(R):
        if r % 3 == 2:
            Y[:, r] = rng.permutation(Y[:, 0])
        else:
            sup = rng.choice(p, 8 + r % 5, replace=False)
            Y[:, r] = X[:, sup] @ (rng.uniform(1.0, 5.0, sup.size) * rng.choice([-1, 1], sup.size)) + rng.standard_normal(n)
    return Y


@pytest.mark.parametrize("variant", ["weights", "always_select"])
def test_multi_equals_single_response_sessions(gpu, variant):
    X, _, _, _ = synth.make_lm(800, 400, 10, seed=21)
    Y = _responses(X, 12, 3)
    seq = np.arange(1, 61)
    kw = dict(weight=np.random.default_rng(4).uniform(0.5, 2.0, 800)) if variant == "weights" else dict(always_select=[3, 77])
    got, cnt = _multi(gpu, X, Y, seq, **kw)
    assert len(got) == 12
    assert cnt["multi_responses_batched"] == 12
    for r, want in enumerate(_singles(gpu, X, Y, seq, **kw)):
        _same(got[r], want, "%s response %d" % (variant, r))


def test_awkward_columns(gpu):
    X, y, sup, _ = synth.make_lm(600, 300, 6, seed=8)
    rng = np.random.default_rng(9)
    near = X[:, sup] @ rng.uniform(1, 3, sup.size) + 1e-3 * rng.standard_normal(600)
    Y = np.column_stack([y, y, -y, rng.standard_normal(600), near, np.full(600, 2.5)])
    seq = np.arange(1, 31)
    singles = []
    for r in range(Y.shape[1]):
        with gpu.Session(X, Y[:, r]) as s:
            try:
                singles.append(s.sequential_path(seq, ic_type=3))
            except gpu.BessxError as e:
                singles.append(e)
    with gpu.Session(X, Y[:, 0]) as s:
        s.set_responses(Y)
        if any(isinstance(o, Exception) for o in singles):
            assert isinstance(singles[-1], Exception) and not any(isinstance(o, Exception) for o in singles[:-1])
            with pytest.raises(gpu.BessxError) as err:
                s.sequential_path_multi(seq, ic_type=3)
            assert err.value.code == singles[-1].code  # (the constant column's own error code)
            Y, singles = Y[:, :-1], singles[:-1]  # (the constant column fails alone as well: the rest still runs)
            s.set_responses(Y)
        got = s.sequential_path_multi(seq, ic_type=3)
    for r, want in enumerate(singles):
        _same(got[r], want, "awkward column %d" % r)


def test_against_the_pinned_oracle(gpu):
    from oracle import port_ctypes as P
    X, _, _, _ = synth.make_lm(400, 120, 5, seed=31)
    Y = _responses(X, 4, 32)
    seq = np.arange(1, 16)
    got, _ = _multi(gpu, X, Y, seq)
    for r in range(Y.shape[1]):
        want = P.trace(X, Y[:, r], ic_type=3, sequence=seq)
        for i, f in enumerate(want["fits"]):
            assert np.array_equal(got[r]["cand_support"][i, :seq[i]], f["iters"][-1]), (r, i)
        assert np.array_equal(np.nonzero(got[r]["beta"])[0], np.nonzero(want["beta"])[0]), r
        np.testing.assert_allclose(got[r]["beta"], want["beta"], rtol=1e-6, atol=1e-9)


def _tie_design():
    X, y, sup, _ = synth.make_lm(300, 40, 5, seed=5)
    X = np.array(X)
    noise = [j for j in range(40) if j not in set(sup)]
    a, b, c = noise[0], noise[3], noise[9]
    X[:, b] = X[:, a]
    X[:, c] = -X[:, a]
    return X, y + 0.6 * X[:, a]


def test_takeover_on_ties_and_ill_conditioned_solves(gpu):
    X, y = _tie_design()
    rng = np.random.default_rng(2)
    Y = np.column_stack([y, y + 0.01 * rng.standard_normal(300), rng.standard_normal(300)])
    seq = np.arange(1, 7)
    got, cnt = _multi(gpu, X, Y, seq)
    assert cnt["multi_responses_batched"] == 3  # (the engine ran all three ...)
    assert cnt["multi_responses_host"] > 0  # ... and the tie at level 6 stopped the device: the host finished those
    for r, want in enumerate(_singles(gpu, X, Y, seq)):
        _same(got[r], want, "ties response %d" % r)
    # nearly collinear columns: ill-conditioned systems whose solves go to the Cholesky kernel
    X2, y2, sup2, _ = synth.make_lm(500, 200, 8, seed=41)
    X2 = np.array(X2)
    for j in range(20, 40):
        X2[:, j] = X2[:, sup2[j % 8]] + 1e-7 * rng.standard_normal(500)
    Y2 = np.column_stack([y2, X2[:, 20:28] @ np.arange(1.0, 9.0) + rng.standard_normal(500)])
    seq2 = np.arange(1, 25)
    got2, cnt2 = _multi(gpu, X2, Y2, seq2)
    # (solves the device hands to the Cholesky kernel stop those responses: the host finishes them)
    assert cnt2["multi_responses_batched"] == 2 and cnt2["multi_responses_host"] > 0 and cnt2["cg_fallbacks"] > 0
    for r, want in enumerate(_singles(gpu, X2, Y2, seq2)):
        _same(got2[r], want, "collinear response %d" % r)


@pytest.mark.parametrize("case", ["lambdas", "streaming", "small_cache"])
def test_where_the_engine_does_not_apply(gpu, monkeypatch, case):
    X, _, _, _ = synth.make_lm(700, 300, 8, seed=51)
    Y = _responses(X, 3, 52)
    seq = np.arange(1, 21)
    lam, kw = (0.0,), {}
    if case == "lambdas":
        lam = (0.0, 0.1)
    elif case == "streaming":
        kw = dict(score_mode=1)
    else:
        helpers.hooks(monkeypatch, cov_cap=128)
    got, cnt = _multi(gpu, X, Y, seq, lam, **kw)
    assert cnt["multi_responses_batched"] == 0 and cnt["multi_responses_host"] == 3
    for r, want in enumerate(_singles(gpu, X, Y, seq, lam, **kw)):
        _same(got[r], want, "%s response %d" % (case, r))


def test_wide_design_where_the_ordinary_path_runs_chunk_chains(gpu):
    """p >= 2048 and >= 96 levels: the ordinary path runs as chunk chains on contexts of their own.  Every route of the
    multi call that goes through it -- one response, a takeover early in a long path, the per-response fallback -- must
    fit the installed response on those contexts too."""
    X, y, _, _ = synth.make_lm(3000, 2048, 20, seed=101)
    Y = np.column_stack([y, _responses(X, 3, 102)[:, 1:]])
    seq = np.arange(1, 101)
    with gpu.Session(X, y) as s:
        s.set_responses(Y[:, 1:2])  # R = 1, a column that is not the session's y
        got = s.sequential_path_multi(seq, ic_type=3)
        cnt = s.counters()
    assert cnt["kpath_chunked_paths"] >= 1 and cnt["multi_responses_host"] == 1
    _same(got[0], _singles(gpu, X, Y[:, 1:2], seq)[0], "R = 1 on chunk chains")
    # max_iter = 2: fits run out of iterations and the device stops the responses early; the host finishes each as a
    # warm link (chunk chains again)
    got, cnt = _multi(gpu, X, Y, seq, max_iter=2)
    assert cnt["multi_responses_batched"] == 3 and cnt["multi_responses_host"] > 0
    for r, want in enumerate(_singles(gpu, X, Y, seq, max_iter=2)):
        _same(got[r], want, "takeover response %d" % r)


def test_parked_chains_are_served_by_union_fills(gpu, monkeypatch):
    """A wide design and a long path (p = 2600, levels 1..160: more columns than a fill speculates on): the chains of
    the merged run park on missing Gram columns in the middle of their paths and are served by union fills -- the
    engine's fill counter says so -- and still return what each response's single chain returns."""
    X, y, _, _ = synth.make_lm(3000, 2600, 60, seed=3)
    Y = np.column_stack([y, _responses(X, 3, 4)[:, 1:]])
    seq = np.arange(1, 161)
    got, cnt = _multi(gpu, X, Y, seq)
    assert cnt["multi_responses_batched"] == 3 and cnt["multi_union_fills"] > 0
    monkeypatch.setenv("BESSX_KPATH_CHAINS", "1")
    for r, want in enumerate(_singles(gpu, X, Y, seq)):
        _same(got[r], want, "parked response %d" % r)


def test_streaming_fallback_on_chunk_chains(gpu):
    X, y, _, _ = synth.make_lm(50000, 2048, 20, seed=111)  # (n p >= 1e8: the streaming form's chunk chains)
    Y = np.column_stack([y, _responses(X, 2, 112)[:, 1:], np.random.default_rng(113).permutation(y)])
    seq = np.arange(1, 61)
    got, cnt = _multi(gpu, X, Y, seq, score_mode=1)
    assert cnt["multi_responses_batched"] == 0 and cnt["multi_responses_host"] == 3 and cnt["kpath_chunked_paths"] >= 1
    for r, want in enumerate(_singles(gpu, X, Y, seq, score_mode=1)):
        _same(got[r], want, "streaming response %d" % r)


def test_session_state_is_restored(gpu):
    X, y, _, _ = synth.make_lm(600, 250, 6, seed=61)
    Y = _responses(X, 5, 62)
    seq = np.arange(1, 26)
    with gpu.Session(X, y) as s:
        before = s.sequential_path(seq, ic_type=3)
        s.set_responses(Y)
        s.sequential_path_multi(seq, ic_type=3)
        after = s.sequential_path(seq, ic_type=3)
    for k in ("cand_support", "cand_iters", "cand_train_loss", "cand_ic", "cand_beta", "cand_coef0", "beta"):
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    assert (after["coef0"], after["ic"], after["train_loss"]) == (before["coef0"], before["ic"], before["train_loss"])


def test_more_responses_than_one_batch(gpu):
    X, _, _, _ = synth.make_lm(300, 64, 4, seed=71)
    Y = _responses(X, 300, 72)
    seq = np.arange(1, 9)
    got, cnt = _multi(gpu, X, Y, seq)
    assert len(got) == 300 and cnt["multi_responses_batched"] + cnt["multi_responses_host"] >= 300
    assert cnt["multi_responses_batched"] == 300
    for r, want in enumerate(_singles(gpu, X, Y, seq)):
        _same(got[r], want, "response %d of 300" % r)


def test_full_size_column_zero_matches_the_compiled_reference(gpu):
    X, y, _, _ = synth.make_lm()
    Y = np.column_stack([y, _responses(X[:, :], 8, 81)[:, 1:]])
    Y[:, 3] = np.random.default_rng(82).permutation(y)
    with gpu.Session(X, y, score_mode=2) as s:
        s.set_responses(Y)
        got = s.sequential_path_multi(np.arange(1, 201), ic_type=3)
        cnt = s.counters()
    assert cnt["multi_responses_batched"] == 8
    g = np.load(GOLD)
    n = helpers.assert_untraced_path_matches_golden(got[0], g, X, 1, "configs[1], response 0 of 8")
    assert n == 200


def test_python_estimators_fit_every_column(gpu):
    X, _, _, _ = synth.make_lm(500, 150, 6, seed=91)
    Y = _responses(X, 4, 92)
    Xt = np.random.default_rng(93).standard_normal((20, 150))
    seq = list(range(1, 16))
    est = linear.PdasLm(sequence=seq)
    est.fit(X, Y)
    assert est.beta.shape == (150, 4) and est.coef0.shape == (4,) and est.ic.shape == (4,)
    assert est.train_loss.shape == (4,) and est.predict(Xt).shape == (20, 4)
    for r in range(4):
        one = linear.PdasLm(sequence=seq)
        one.fit(X, Y[:, r])
        np.testing.assert_allclose(est.beta[:, r], one.beta, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose([est.coef0[r], est.train_loss[r], est.ic[r]],
                                   np.ravel([one.coef0, one.train_loss, one.ic]), rtol=1e-9)
        np.testing.assert_allclose(est.predict(Xt)[:, r], one.predict(Xt), rtol=1e-9, atol=1e-9)
    for kw in (dict(path_type="pgs", s_min=1, s_max=10), dict(sequence=seq, is_cv=True, K=3)):
        many = linear.PdasLm(**kw)
        many.fit(X, Y[:, :2])
        for r in range(2):
            one = linear.PdasLm(**kw)
            one.fit(X, Y[:, r])
            np.testing.assert_allclose(many.beta[:, r], one.beta, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(many.coef0[r], np.ravel(one.coef0)[0], rtol=1e-9, atol=1e-12)
