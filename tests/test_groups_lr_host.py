"""Grouped acquisition by log ratio, host side (no GPU): the two entry points' signatures and argument checks (every
check precedes the first launch), the flag constant, and the validation of ``score``."""
import types

import pytest

P = 4096  # non-null placeholders are never dereferenced: every check precedes the launch


def test_symbols_and_flag():
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    L = N.lib()
    for name, nargs in {"hbx_kde_acquire_groups_batch_lr": 20, "hbx_kde_propose_groups_lr": 29}.items():
        assert hasattr(L, name) and len(N.SIGNATURES[name][1]) == nargs, name
    hdr = open(__file__.replace("tests/test_groups_lr_host.py", "include/hbx.h")).read()
    assert "#define HBX_ACQ_LOG_RATIO %d " % groups.ACQ_LOG_RATIO in hdr and groups.ACQ_LOG_RATIO == 2 * groups.ACQ_SKIPPED
    assert L.hbx_version().decode().startswith("hbx 0.3.")


def test_acquire_lr_checks_its_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()

    def acq(X=P, D=3, B=4, S=3, C=8, want=P, res=P, ws=P, wsb=1 << 30):
        return L.hbx_kde_acquire_groups_batch_lr(X or None, D, P, B, P, P, P, P, P, P, P, P, P, S, C, want or None,
                                                 res or None, ws or None, wsb, None)

    assert acq(X=0) == -1 and b"hbx_kde_acquire_groups_batch_lr" in L.hbx_last_error()
    assert acq(res=0) == -1 and acq(ws=0) == -1 and acq(B=-1) == -1 and acq(S=-1) == -1 and acq(C=-1) == -1
    assert acq(D=0) == -1 and acq(D=257) == -1 and b"D=" in L.hbx_last_error()
    assert acq(B=1 << 12, S=1 << 10, C=1 << 10) == -1 and b"int32" in L.hbx_last_error()
    assert acq(wsb=L.hbx_kde_groups_batch_workspace_bytes(4, 3, 8, 3) - 1) == -1 and b"too small" in L.hbx_last_error()
    assert acq(ws=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert acq(B=0) == 0 and acq(S=0) == 0 and acq(B=0, want=0, res=0, ws=0) == 0


def test_propose_lr_checks_its_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()

    def prop(X=P, lv=P, D=3, B=4, S=3, C=8, rf=0.25, want=P, flags=0, rows=P, src=P, ws=P, wsb=1 << 30, cands=None):
        return L.hbx_kde_propose_groups_lr(X or None, D, P, B, P, P, P, P, P, P, P, P, lv or None, 3.0, rf, 1, 0, 0, S,
                                           C, want or None, flags, rows or None, src or None, None, cands, ws or None,
                                           wsb, None)

    assert prop(X=0) == -1 and b"hbx_kde_propose_groups_lr" in L.hbx_last_error()
    assert prop(lv=0) == -1 and prop(rows=0) == -1 and prop(src=0) == -1 and prop(ws=0) == -1 and prop(C=0) == -1
    assert prop(D=0) == -1 and prop(D=257) == -1 and prop(flags=2) == -1 and b"flags" in L.hbx_last_error()
    assert prop(rf=-1.0) == -1 and prop(B=1 << 12, S=1 << 10, C=1 << 10) == -1
    assert prop(wsb=L.hbx_kde_propose_groups_m_workspace_bytes(4, 3, 8, 3) - 1) == -1
    assert b"too small" in L.hbx_last_error()
    assert prop(ws=4104) == -1 and prop(cands=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert prop(B=0) == 0 and prop(S=0, flags=1, want=0) == 0


def test_score_is_validated():
    from hpbandster_amd import groups
    gm = types.SimpleNamespace()  # the check comes first: nothing of the model is read
    with pytest.raises(ValueError, match="score"):
        groups.GroupModel.acquire_requests(gm, None, score="bogus")
    with pytest.raises(ValueError, match="score"):
        groups.GroupModel.get_config(gm, 8, 0, [0, 0], score="bogus")
    with pytest.raises(ValueError, match="score"):
        groups.GroupBOHB(2, "cc", [0, 0], score="bogus")
    assert groups.GroupBOHB(2, "cc", [0, 0], device="cuda:0").score == "ratio"  # (the device is only stored)
    assert groups.GroupBOHB(2, "cc", [0, 0], device="cuda:0", score="log_ratio").score == "log_ratio"
