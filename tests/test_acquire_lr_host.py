"""Single-pool acquisition by log ratio, host side (no GPU): the validation of ``score`` and of what it excludes, the
native calls' argument checks (every check precedes the first launch) and the workspace size helper."""
import types

import pytest

P = 4096  # non-null placeholders are never dereferenced: every check precedes the launch


def test_score_is_validated():
    from hpbandster_amd import kde
    from hpbandster_amd.config_generators.bohb import BOHB
    pair = types.SimpleNamespace()  # the checks come first: nothing of the pair is read
    for kw in ({"score": "bogus"}, {"score": "log_ratio", "logs": True}, {"score": "log_ratio", "ties": "process"}):
        with pytest.raises(ValueError, match="score"):
            kde.KDEPair.acquire(pair, None, **kw)
    for call in (lambda: kde.KDEPair.acquire_pick(pair, None, None, None, None, score="bogus"),
                 lambda: kde.KDEPair.acquire_mapped(pair, None, score="bogus"),
                 lambda: kde.KDEPair.workspace_bytes(pair, 64, score="bogus"), lambda: BOHB(None, score="bogus")):
        with pytest.raises(ValueError, match="score"):
            call()
    cg = BOHB.__new__(BOHB)
    cg.score, cg.speculative, cg.sampler = "log_ratio", "always", "gpu"
    assert not cg.speculation_enabled()
    for call in (lambda: cg.get_config_batch(1.0, 2), lambda: cg.get_config_topk(1.0, 2)):
        with pytest.raises(ValueError, match="score"):
            call()
    cg.score = "floored"
    assert cg.speculation_enabled()


def test_native_calls_check_their_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name, nargs in {"hbx_kde_lr_workspace_bytes": 2, "hbx_kde_acquire_lr": 8, "hbx_kde_acquire_bound_lr": 11}.items():
        assert hasattr(L, name) and len(N.SIGNATURES[name][1]) == nargs, name
    pair = L.hbx_kde_pair_bind(3, P, P, P, P, 0, P, P, P, P, 0, 4, 0, 400)
    assert pair
    big, small = L.hbx_kde_lr_workspace_bytes(64, 400), L.hbx_kde_workspace_bytes(64, 400)
    assert big >= small and L.hbx_kde_lr_workspace_bytes(0, 0) >= L.hbx_kde_workspace_bytes(0, 0)

    def acq(pair=pair, cand=P, ws=P, wsb=big):
        return L.hbx_kde_acquire_lr(cand or None, 64, 0, pair or None, ws or None, wsb, None, None)

    def bound(pair=pair, cand=P, ws=P, wsb=big, rec=P):
        return L.hbx_kde_acquire_bound_lr(pair or None, cand or None, 64, 0, ws or None, wsb, None, None, None,
                                          rec or None, None)

    try:
        assert acq(pair=0) == -1 and b"hbx_kde_acquire_lr" in L.hbx_last_error()
        assert acq(cand=0) == -1 and acq(ws=0) == -1 and b"null" in L.hbx_last_error()
        assert acq(wsb=small - 1) == -1 and b"too small" in L.hbx_last_error()
        assert bound(pair=0) == -1 and bound(rec=0) == -1 and b"hbx_kde_acquire_bound_lr" in L.hbx_last_error()
    finally:
        L.hbx_kde_pair_free(pair)
