"""Who owns the GPU-side resources of a session: every device buffer, pinned buffer and event of the library is handed
out by an owner (bessx_host.h: Owner) that gives all of it back when the session, the CV folds or a fit context go.

The ledger (bessx_session_counter 38 / 39: live device / pinned bytes of the PROCESS, 40: allocation requests so far)
counts the library's own requests only, so it does not depend on who else uses the card: after a session is destroyed
both byte counts must be back EXACTLY where they were.  BESSX_TEST_HOOKS=alloc_fail=N makes the N-th request after
the hook was set fail on the host (hipErrorOutOfMemory without a call to the runtime; nothing is launched
differently): walking N over an operation exercises every clean-up path it has."""
import os

import numpy as np
import pytest

from bess_amd import synth

pytestmark = pytest.mark.gpu

WALK_MAX = 2000
KEYS_EXACT = ("cand_T0", "cand_support", "cand_iters", "cand_beta", "cand_ic", "cand_train_loss")


@pytest.fixture(scope="module")
def probe(gpu):
    """One tiny session that stays open: the ledger is read through it."""
    X, y, _, _ = synth.make_lm(64, 8, 2, seed=1)
    s = gpu.Session(X, y)
    yield s
    s.close()


def ledger(probe):
    c = probe.counters()
    return c["live_device_bytes_of_the_process"], c["live_pinned_bytes_of_the_process"]


def requests(probe):
    return probe.counters()["allocation_requests_of_the_process"]


def set_alloc_fail(n):
    """alloc_fail=n beside whatever other hooks are set (n = None: the hook removed)."""
    cur = dict(kv.split("=", 1) for kv in os.environ.get("BESSX_TEST_HOOKS", "").split(",") if "=" in kv)
    cur.pop("alloc_fail", None)
    if n is not None:
        cur["alloc_fail"] = str(n)
    if cur:
        os.environ["BESSX_TEST_HOOKS"] = ",".join("%s=%s" % kv for kv in cur.items())
    else:
        os.environ.pop("BESSX_TEST_HOOKS", None)


@pytest.fixture
def alloc_fail():
    keep = os.environ.get("BESSX_TEST_HOOKS")
    yield set_alloc_fail
    if keep is None:
        os.environ.pop("BESSX_TEST_HOOKS", None)
    else:
        os.environ["BESSX_TEST_HOOKS"] = keep


def same(a, b, what=""):
    for k in KEYS_EXACT:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


def group_index(p, width):
    return np.arange(0, p, width, dtype=np.int32)


# ---- 1. everything comes back --------------------------------------------------------------------------------------
def _lm(gpu, monkeypatch):
    X, y, _, _ = synth.make_lm(1500, 400, 8, seed=4)
    with gpu.Session(X, y) as s:
        assert s.score_mode() == 2
        s.sequential_path(np.arange(1, 25), ic_type=3)
        s.gs_path(1, 20, ic_type=3)


def _lm_streaming(gpu, monkeypatch):
    monkeypatch.setenv("BESSX_SCORE_MODE", "1")
    X, y, _, _ = synth.make_lm(1500, 400, 8, seed=4)
    with gpu.Session(X, y) as s:
        assert s.score_mode() == 1
        s.sequential_path(np.arange(1, 25), ic_type=3)


def _logistic(gpu, monkeypatch):
    X, y, _, _ = synth.make_logistic(1500, 300, 8, seed=4)
    with gpu.Session(X, y, data_type=2, model_type=2) as s:
        s.sequential_path(np.arange(1, 16), ic_type=3)


def _poisson(gpu, monkeypatch):
    X, y, _, _ = synth.make_poisson(1500, 300, 8, seed=4)
    with gpu.Session(X, y, data_type=2, model_type=3) as s:
        s.sequential_path(np.arange(1, 12), ic_type=3)


def _cox(gpu, monkeypatch):
    X, _, st, _, _ = synth.make_cox(1500, 300, 8)
    with gpu.Session(X, st, data_type=3, model_type=4) as s:
        s.sequential_path(np.arange(1, 12), ic_type=3)


def _lm_grouped(gpu, monkeypatch):
    X, y, _, _ = synth.make_lm(1200, 240, 8, seed=5)
    for width, kw in ((4, {}), (4, dict(score_mode=1)), (24, {})):  # diagonalised blocks (both score forms), Cholesky form
        with gpu.Session(X, y, algorithm_type=2, g_index=group_index(240, width), **kw) as s:
            s.sequential_path(np.arange(1, 7), ic_type=3)
            s.set_cv(3, synth.make_cv_folds(1200, 3))
            s.sequential_path(np.arange(1, 5), ic_type=3, is_cv=True)


def _screening(gpu, monkeypatch):
    X, y, _, _ = synth.make_lm(1000, 400, 8, seed=6)
    with gpu.Session(X, y, is_screening=True, screening_size=60) as s:
        s.sequential_path(np.arange(1, 12), ic_type=3)
    Xl, yl, _, _ = synth.make_logistic(1000, 120, 6, seed=6)
    with gpu.Session(Xl, yl, data_type=2, model_type=2, is_screening=True, screening_size=40) as s:
        s.sequential_path(np.arange(1, 8), ic_type=3)


def _screening_wide_groups(gpu, monkeypatch):
    # groups of 12 columns: wider than the 8 (logistic) / 4 (Cox) a block of the screening kernel fits -- every group is
    # fitted in a sub-session of its own
    Xl, yl, _, _ = synth.make_logistic(800, 120, 6, seed=7)
    with gpu.Session(Xl, yl, data_type=2, model_type=2, algorithm_type=2, g_index=group_index(120, 12),
                     is_screening=True, screening_size=4) as s:
        s.sequential_path(np.arange(1, 4), ic_type=3)
    Xc, _, st, _, _ = synth.make_cox(800, 120, 6)
    with gpu.Session(Xc, st, data_type=3, model_type=4, algorithm_type=2, g_index=group_index(120, 12),
                     is_screening=True, screening_size=4) as s:
        s.sequential_path(np.arange(1, 4), ic_type=3)
    Xg, yg, _, _ = synth.make_lm(800, 120, 6, seed=7)
    with gpu.Session(Xg, yg, algorithm_type=2, g_index=group_index(120, 12), is_screening=True, screening_size=4) as s:
        s.sequential_path(np.arange(1, 4), ic_type=3)


def _cv(gpu, monkeypatch):
    X, y, _, _ = synth.make_lm(1500, 400, 8, seed=4)
    with gpu.Session(X, y) as s:
        s.set_cv(4, synth.make_cv_folds(1500, 4))
        assert s.counters()["cv_fold_contexts"] > 0
        s.sequential_path(np.arange(1, 21), ic_type=3, is_cv=True)
    Xl, yl, _, _ = synth.make_logistic(1200, 200, 6, seed=4)
    with gpu.Session(Xl, yl, data_type=2, model_type=2) as s:
        s.set_cv(3, synth.make_cv_folds(1200, 3))
        s.sequential_path(np.arange(1, 9), ic_type=3, is_cv=True)


def _cv_twice(gpu, monkeypatch):
    X, y, _, _ = synth.make_lm(1500, 400, 8, seed=4)
    with gpu.Session(X, y) as s:
        s.set_cv(3, synth.make_cv_folds(1500, 3))
        s.sequential_path(np.arange(1, 11), ic_type=3, is_cv=True)
        s.set_cv(5, synth.make_cv_folds(1500, 5))
        assert s.counters()["cv_fold_contexts"] == 5
        s.sequential_path(np.arange(1, 11), ic_type=3, is_cv=True)
        s.sequential_path(np.arange(1, 11), ic_type=3)


def _chunked(gpu, monkeypatch):
    X, y, _, _ = synth.make_lm(2000, 500, 10)
    for kw in ({}, dict(score_mode=1)):
        with gpu.Session(X, y, **kw) as s:
            s.set_kpath_chains(2)
            s.sequential_path(np.arange(1, 21), ic_type=3)
            s.set_kpath_chains(3)
            s.sequential_path(np.arange(1, 31), ic_type=3)
            assert s.counters()["kpath_chunked_paths"] == 2
    Xl, yl, _, _ = synth.make_logistic(1500, 300, 8, seed=4)
    with gpu.Session(Xl, yl, data_type=2, model_type=2) as s:
        s.set_kpath_chains(2)
        s.sequential_path(np.arange(1, 17), ic_type=3)
        assert s.counters()["kpath_chunked_paths"] == 1
    Xc, _, st, _, _ = synth.make_cox(1500, 300, 8)
    with gpu.Session(Xc, st, data_type=3, model_type=4) as s:
        s.set_kpath_chains(2)
        s.sequential_path(np.arange(1, 13), ic_type=3)
        assert s.counters()["kpath_chunked_paths"] == 1


def _multi_response(gpu, monkeypatch):
    X, y, _, _ = synth.make_lm(1500, 400, 8, seed=4)
    rng = np.random.default_rng(3)
    with gpu.Session(X, y) as s:
        for R in (3, 6):
            Y = X[:, :R] * 2.0 + X[:, 10:10 + R] + 0.1 * rng.standard_normal((1500, R))
            s.set_responses(Y)
            assert len(s.sequential_path_multi(np.arange(1, 13), ic_type=3)) == R
        assert s.counters()["multi_responses_batched"] > 0
        s.sequential_path(np.arange(1, 13), ic_type=3)


def _device_input(gpu, monkeypatch):
    import torch
    X, y, _, _ = synth.make_lm(1500, 400, 8, seed=4)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    yd = torch.from_numpy(y).cuda()
    with gpu.Session(Xd, yd, row_order=np.arange(1500)[::-1].copy()) as s:
        s.sequential_path(np.arange(1, 21), ic_type=3)
        s.set_responses(torch.from_numpy(np.stack([y, -y], axis=1)).cuda())
        s.sequential_path_multi(np.arange(1, 9), ic_type=3)
    with gpu.Session(Xd, y, is_screening=True, screening_size=50) as s:
        s.sequential_path(np.arange(1, 9), ic_type=3)
    torch.cuda.synchronize()


CASES = [_lm, _lm_streaming, _logistic, _poisson, _cox, _lm_grouped, _screening, _screening_wide_groups, _cv, _cv_twice,
         _chunked, _multi_response, _device_input]


@pytest.mark.parametrize("case", CASES, ids=[c.__name__.lstrip("_") for c in CASES])
def test_everything_comes_back(gpu, probe, monkeypatch, case):
    base = ledger(probe)
    case(gpu, monkeypatch)
    assert ledger(probe) == base, "live (device, pinned) bytes after the sessions are gone"


def test_the_ledger_sees_a_live_session(gpu, probe):
    """(the check above would pass on a ledger that counts nothing)"""
    base = ledger(probe)
    X, y, _, _ = synth.make_lm(1500, 400, 8, seed=4)
    with gpu.Session(X, y) as s:
        dev, pin = ledger(probe)
        assert dev - base[0] >= 1536 * 400 * 8 and pin > base[1]  # at least the padded X; the pinned result blocks
        s.set_cv(3, synth.make_cv_folds(1500, 3))
        assert ledger(probe)[0] > dev
    assert ledger(probe) == base


# ---- 2. a failed allocation leaves nothing behind and breaks nothing ---------------------------------------------------
@pytest.mark.parametrize("fam", ["lm", "lm-screening", "cox"])
def test_failed_allocation_during_creation(gpu, probe, alloc_fail, fam):
    if fam == "cox":
        X, _, y, _, _ = synth.make_cox(600, 90, 4)
        kw, seq = dict(data_type=3, model_type=4), np.arange(1, 6)
    else:
        X, y, _, _ = synth.make_lm(600, 120, 5, seed=8)
        kw, seq = (dict(is_screening=True, screening_size=40) if fam == "lm-screening" else {}), np.arange(1, 11)

    def run():
        with gpu.Session(X, y, **kw) as s:
            return s.sequential_path(seq, ic_type=3)

    want = run()
    base = ledger(probe)
    for N in range(1, WALK_MAX + 1):
        before = requests(probe)
        alloc_fail(N)
        try:
            s = gpu.Session(X, y, **kw)
        except gpu.BessxError as e:
            s = None
            msg = str(e)
        finally:
            alloc_fail(None)
        fired = requests(probe) - before >= N
        if s is not None:  # creation succeeded, which ends the walk: the hook was set beyond its last request
            s.close()
            assert not fired, "request %d failed and the session was created all the same" % N
            assert ledger(probe) == base
            break
        assert fired and gpu.last_error() and msg, "N = %d" % N
        assert ledger(probe) == base, "N = %d: a failed creation left (device, pinned) bytes behind" % N
        same(run(), want, "the session created after failure %d" % N)
    else:
        pytest.fail("the walk over session creation has not ended after %d steps" % WALK_MAX)
    assert N > 20  # (a session makes far more requests than that: the hook was really walked)


def test_failed_allocation_during_set_cv(gpu, probe, alloc_fail, monkeypatch):
    """set_cv on a live session: an error leaves the session fitting without CV exactly as before; a failure while the
    fold-major copy is allocated leaves the masked per-row-set fills in place (what cv_shared=0 selects), one inside the
    fold contexts leaves the folds running one after another (counter 11; what cv_side_by_side=0 selects)."""
    from helpers import hooks
    X, y, _, _ = synth.make_lm(900, 150, 6, seed=9)
    K, folds, seq = 3, synth.make_cv_folds(900, 3), np.arange(1, 11)

    def cv_reference(**hk):
        with monkeypatch.context() as m:
            hooks(m, **hk)
            with gpu.Session(X, y) as s:
                s.set_cv(K, folds)
                return s.sequential_path(seq, ic_type=3, is_cv=True)

    want_one_by_one = cv_reference(cv_side_by_side=0)
    want_unshared = cv_reference(cv_shared=0)
    base = ledger(probe)
    with gpu.Session(X, y) as s:
        want_nocv = s.sequential_path(seq, ic_type=3)
        live = ledger(probe)
        for N in range(1, WALK_MAX + 1):
            dropped, before = s.counters()["cv_contexts_dropped"], requests(probe)
            alloc_fail(N)
            try:
                s.set_cv(K, folds)
                err = None
            except gpu.BessxError as e:
                err = str(e)
            finally:
                alloc_fail(None)
            fired = requests(probe) - before >= N
            c = s.counters()
            if err is not None:
                assert fired and err and gpu.last_error(), "N = %d" % N
                assert ledger(probe) == live, "N = %d: a failed set_cv left (device, pinned) bytes behind" % N
                same(s.sequential_path(seq, ic_type=3), want_nocv, "without CV after failure %d" % N)
                continue
            got = s.sequential_path(seq, ic_type=3, is_cv=True)
            if not fired:  # the whole of set_cv went through: the walk ends
                assert c["cv_fold_contexts"] == K and c["cv_contexts_dropped"] == dropped
                break
            assert c["cv_fold_contexts"] == 0, "N = %d" % N
            if c["cv_contexts_dropped"] == dropped + 1:
                same(got, want_one_by_one, "folds one after another after failure %d" % N)
            else:
                assert c["cv_contexts_dropped"] == dropped and N <= 3, "N = %d" % N  # (Xp, zp, cvp_part)
                same(got, want_unshared, "masked fills after failure %d" % N)
        else:
            pytest.fail("the walk over set_cv has not ended after %d steps" % WALK_MAX)
        assert N > 20
    assert ledger(probe) == base


@pytest.mark.parametrize("form", ["covariance", "streaming"])
def test_failed_allocation_during_first_chunked_path(gpu, probe, alloc_fail, form):
    """The first chunked path of a session creates the chain contexts, the host threads' rendezvous and the buffers of
    the merged launches / shared passes: the call either fails cleanly or falls back (fewer mechanisms, same path).  After
    a call that failed, the same session walks the same path again: nothing of the failed call (members of a shared-pass
    round, launch counters, a half-made context) is left for it to trip over."""
    X, y, _, _ = synth.make_lm(1200, 300, 8, seed=10)
    kw, seq = (dict(score_mode=1) if form == "streaming" else {}), np.arange(1, 21)
    with gpu.Session(X, y, **kw) as s:
        s.set_kpath_chains(2)
        want = s.sequential_path(seq, ic_type=3)
        assert s.counters()["kpath_chunked_paths"] == 1
    base = ledger(probe)
    for N in range(1, WALK_MAX + 1):
        with gpu.Session(X, y, **kw) as s:
            s.set_kpath_chains(2)
            before = requests(probe)
            alloc_fail(N)
            try:
                got, err = s.sequential_path(seq, ic_type=3), None
            except gpu.BessxError as e:
                got, err = None, str(e)
            finally:
                alloc_fail(None)
            fired = requests(probe) - before >= N
            if err is not None:
                assert fired and err and gpu.last_error(), "N = %d" % N
                # the SAME session, the hook removed: the failed call left nothing behind that its next path trips over
                paths = s.counters()["kpath_chunked_paths"]
                again = s.sequential_path(seq, ic_type=3)
                assert np.array_equal(again["cand_support"], want["cand_support"]), "N = %d, same session" % N
                assert np.allclose(again["cand_ic"], want["cand_ic"], rtol=1e-9), "N = %d, same session" % N
                # (as chunk chains again, or -- contexts not to be had -- the same path as one chain)
                assert s.counters()["kpath_chunked_paths"] in (paths, paths + 1), "N = %d, same session" % N
            else:
                assert np.array_equal(got["cand_support"], want["cand_support"]), "N = %d" % N
                assert np.allclose(got["cand_ic"], want["cand_ic"], rtol=1e-9), "N = %d" % N
                if not fired:
                    assert s.counters()["kpath_chunked_paths"] == 1
        assert ledger(probe) == base, "N = %d: (device, pinned) bytes left after the session was destroyed" % N
        if not fired:
            break
    else:
        pytest.fail("the walk over the first chunked path has not ended after %d steps" % WALK_MAX)
    assert N > 20
