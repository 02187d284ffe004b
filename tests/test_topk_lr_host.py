"""Single-pool top-k by log ratio, host side (no GPU): the validation of ``score``, the new entry points' signatures and argument checks (every check precedes the first launch)."""
import types

import pytest

P = 4096  # non-null placeholders are never dereferenced: every check precedes the launch


def test_score_is_validated():
    from hpbandster_amd import kde
    pair = types.SimpleNamespace()  # the checks come first: nothing of the pair is read
    for call in (lambda: kde.KDEPair.acquire_topk(pair, None, 4, score="bogus"),
                 lambda: kde.KDEPair.topk_workspace_bytes(pair, 64, 4, score="bogus")):
        with pytest.raises(ValueError, match="score"):
            call()


def test_native_calls_check_their_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name, nargs in {"hbx_kde_topk_lr_workspace_bytes": 3, "hbx_kde_acquire_topk_lr": 9}.items():
        assert hasattr(L, name) and len(N.SIGNATURES[name][1]) == nargs, name
    f = L.hbx_kde_topk_lr_workspace_bytes
    assert f(64, 8, 400) >= L.hbx_kde_lr_workspace_bytes(64, 400) + 4 * 1024
    assert f(64, 0, 400) == -1 and f(64, 1025, 400) == -1 and f(-1, 8, 400) == -1 and f(0, 8, 0) > 0
    pair = L.hbx_kde_pair_bind(3, P, P, P, P, 0, P, P, P, P, 0, 4, 0, 400)
    assert pair

    def acq(pair=pair, cand=P, k=8, res=P, ws=P, wsb=f(64, 8, 400)):
        return L.hbx_kde_acquire_topk_lr(cand or None, 64, k, 0, pair or None, res or None, ws or None, wsb, None)

    try:
        assert acq(pair=0) == -1 and b"hbx_kde_acquire_topk_lr" in L.hbx_last_error()
        assert acq(cand=0) == -1 and acq(ws=0) == -1 and acq(res=0) == -1 and b"null" in L.hbx_last_error()
        assert acq(k=0) == -1 and acq(k=1025) == -1 and b"outside" in L.hbx_last_error()
        assert acq(wsb=f(64, 8, 400) - 1) == -1 and b"too small" in L.hbx_last_error()
    finally:
        L.hbx_kde_pair_free(pair)
