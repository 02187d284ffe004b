"""The request mask of the grouped get_config calls, host side (no GPU): the new entry points' signatures and
argument checks (every check precedes the first launch), the counts-to-mask rule, SOURCE_SKIPPED, and the validation
of ``fills`` and ``skip_random``."""
import numpy as np
import pytest

NEW = {"hbx_kde_sample_groups_m": 18, "hbx_kde_acquire_groups_batch_m": 21, "hbx_kde_groups_request_stats": 2,
       "hbx_kde_finish_groups_m": 16, "hbx_kde_random_requests_groups": 10,
       "hbx_kde_propose_groups_m_workspace_bytes": 4, "hbx_kde_propose_groups_m_ws_offsets": 5,
       "hbx_kde_propose_groups_m": 30}


def test_new_symbols_have_signatures():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name, nargs in NEW.items():
        assert hasattr(L, name) and name in N.SIGNATURES, name
        assert len(N.SIGNATURES[name][1]) == nargs, name


def test_constants():
    from hpbandster_amd import groups
    assert groups.SOURCE_SKIPPED == 5 and groups.GroupConfigs.SOURCE_SKIPPED == 5
    assert groups.ACQ_SKIPPED == 64 and groups.PROPOSE_SKIP_RANDOM == 1
    hdr = open(__file__.replace("tests/test_groups_mask_host.py", "include/hbx.h")).read()
    for line in ("#define HBX_ACQ_SKIPPED 64", "#define HBX_CFG_SKIPPED 5", "#define HBX_PROPOSE_SKIP_RANDOM 1"):
        assert line in hdr, line
    cfg = groups.GroupConfigs(np.zeros((2, 3, 4)), np.array([[0, 5, 1], [5, 0, 2]], dtype=np.uint8), 2, 3)
    np.testing.assert_array_equal(cfg.model_based, [[True, False, False], [False, True, False]])


def test_counts_to_mask():
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    m = groups.counts_to_mask(np.array([0, 4, 1, 9, -2]), 4)
    assert m.dtype == np.uint8
    np.testing.assert_array_equal(m, [[0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 0]])
    assert groups.counts_to_mask(np.zeros(0, dtype=np.int64), 3).shape == (0, 3)
    assert groups.counts_to_mask(np.array([2], dtype=np.int32), 0).shape == (1, 0)
    for bad in (np.array([1.0, 2.0]), np.ones((2, 2), dtype=np.int64)):
        with pytest.raises(N.HbxError):
            groups.counts_to_mask(bad, 3)
    import torch
    t = groups.counts_to_mask(torch.tensor([0, 3, 1]), 3)  # the tensor form: the same rule where the counts lie
    assert t.dtype == torch.uint8
    np.testing.assert_array_equal(t.numpy(), [[0, 0, 0], [1, 1, 1], [1, 0, 0]])
    with pytest.raises(N.HbxError):
        groups.counts_to_mask(torch.tensor([0.5, 1.0]), 3)


def test_request_mask_refuses_before_any_device_work():
    from hpbandster_amd import _native as N
    from hpbandster_amd import groups
    import torch
    assert groups.request_mask(None, 3, 4, "cuda:0") is None
    bad = [np.ones((3, 4)), np.ones((3, 5), dtype=np.uint8), np.ones((4, 3), dtype=bool), np.ones(4, dtype=np.int64),
           np.ones((3, 4), dtype=np.int32), np.ones(3), torch.ones((3, 4), dtype=torch.uint8),  # (a host tensor)
           torch.ones(3, dtype=torch.int64)]
    for w in bad:
        with pytest.raises(N.HbxError):
            groups.request_mask(w, 3, 4, "cuda:0")


def test_entry_points_check_their_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()
    p = 4096  # non-null placeholders are never dereferenced: every check precedes the launch

    def smp(X=p, D=3, B=4, S=3, C=8, want=p, cands=p):
        return L.hbx_kde_sample_groups_m(X or None, D, p, B, p, p, p, p, 3.0, 1, 0, 0, S, C, want or None, cands or None,
                                         None, None)

    assert smp(X=0) == -1 and b"hbx_kde_sample_groups_m" in L.hbx_last_error()
    assert smp(cands=0) == -1 and smp(D=0) == -1 and smp(B=-1) == -1 and smp(S=-1) == -1 and smp(C=-1) == -1
    assert smp(B=1 << 12, S=1 << 10, C=1 << 10) == -1 and b"int32" in L.hbx_last_error()
    assert smp(D=4, cands=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert smp(B=0) == 0 and smp(S=0) == 0 and smp(C=0) == 0 and smp(B=0, want=0) == 0

    def acq(X=p, D=3, B=4, S=3, C=8, want=p, res=p, ws=p, wsb=1 << 30):
        return L.hbx_kde_acquire_groups_batch_m(X or None, D, p, B, p, p, p, p, p, p, p, p, p, S, C, want or None,
                                                res or None, ws or None, wsb, None, None)

    assert acq(X=0) == -1 and b"hbx_kde_acquire_groups_batch_m" in L.hbx_last_error()
    assert acq(res=0) == -1 and acq(ws=0) == -1 and acq(D=0) == -1 and acq(B=-1) == -1 and acq(S=-1) == -1
    assert acq(B=1 << 12, S=1 << 10, C=1 << 10) == -1 and b"int32" in L.hbx_last_error()
    assert acq(wsb=L.hbx_kde_groups_batch_workspace_bytes(4, 3, 8, 3) - 1) == -1 and b"too small" in L.hbx_last_error()
    assert acq(ws=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert acq(B=0) == 0 and acq(S=0) == 0

    def fin(rec=p, cands=p, lv=p, D=3, B=4, S=3, C=8, rf=0.25, want=p, rows=p, src=p):
        return L.hbx_kde_finish_groups_m(rec or None, cands or None, p, lv or None, D, B, S, C, rf, 1, 0, 0,
                                         want or None, rows or None, src or None, None)

    assert fin(lv=0) == -1 and b"hbx_kde_finish_groups_m" in L.hbx_last_error()
    assert fin(rows=0) == -1 and fin(src=0) == -1 and fin(cands=0) == -1 and fin(C=0) == -1 and fin(D=257) == -1
    assert fin(rf=1.5) == -1 and b"random_fraction" in L.hbx_last_error()
    assert fin(B=0) == 0 and fin(S=0) == 0

    def rnd(B=4, S=3, C=8, rf=0.25, out=p):
        return L.hbx_kde_random_requests_groups(B, S, C, rf, 1, 0, 0, None, out or None, None)

    assert rnd(out=0) == -1 and b"hbx_kde_random_requests_groups" in L.hbx_last_error()
    assert rnd(B=-1) == -1 and rnd(C=0) == -1 and rnd(B=1 << 12, S=1 << 10, C=1 << 10) == -1
    for bad in (-0.01, 1.01, float("nan")):
        assert rnd(rf=bad) == -1 and b"random_fraction" in L.hbx_last_error()
    assert rnd(B=0) == 0 and rnd(S=0, out=0) == 0
    assert L.hbx_kde_groups_request_stats(None, None) == -1


def test_propose_m_workspace_and_checks():
    from hpbandster_amd import _native as N
    L = N.lib()
    f, g = L.hbx_kde_propose_groups_m_workspace_bytes, L.hbx_kde_propose_groups_workspace_bytes
    B, S, C, D = 10, 4, 64, 32
    assert f(B, S, C, D) == g(B, S, C, D) + 48  # the effective mask, B * S bytes in 16-byte steps
    off4, off5 = np.zeros(4, dtype=np.int64), np.zeros(5, dtype=np.int64)
    assert L.hbx_kde_propose_groups_ws_offsets(B, S, C, D, off4.ctypes.data) == 0
    assert L.hbx_kde_propose_groups_m_ws_offsets(B, S, C, D, off5.ctypes.data) == 0
    assert list(off5[:4]) == list(off4) and off5[4] == f(B, S, C, D)
    assert f(10, 4, 0, 32) == -1 and f(1, 1, 1, 257) == -1 and f(1 << 12, 1 << 10, 1 << 10, 32) == -1
    assert L.hbx_kde_propose_groups_m_ws_offsets(B, S, C, D, None) == -1
    p = 4096

    def prop(X=p, lv=p, D=3, B=4, S=3, C=8, rf=0.25, want=p, flags=0, rows=p, src=p, ws=p, wsb=1 << 30, cands=None):
        return L.hbx_kde_propose_groups_m(X or None, D, p, B, p, p, p, p, p, p, p, p, lv or None, 3.0, rf, 1, 0, 0, S,
                                          C, want or None, flags, rows or None, src or None, None, cands, ws or None,
                                          wsb, None, None)

    assert prop(X=0) == -1 and b"hbx_kde_propose_groups_m" in L.hbx_last_error()
    assert prop(lv=0) == -1 and prop(rows=0) == -1 and prop(src=0) == -1 and prop(ws=0) == -1 and prop(C=0) == -1
    assert prop(flags=2) == -1 and b"flags" in L.hbx_last_error()
    assert prop(rf=-1.0) == -1 and prop(B=1 << 12, S=1 << 10, C=1 << 10) == -1
    assert prop(wsb=f(4, 3, 8, 3) - 1) == -1 and b"too small" in L.hbx_last_error()
    assert prop(ws=4104) == -1 and prop(cands=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert prop(B=0) == 0 and prop(S=0, flags=1) == 0


def test_fills_and_skip_random_are_validated():
    from hpbandster_amd import groups
    assert groups.GroupSuccessiveHalving([3, 1], [1, 3]).fills == "all"
    assert groups.GroupSuccessiveHalving([3, 1], [1, 3], fills="needed").fills == "needed"
    for bad in ("some", None, True, 1):
        with pytest.raises(ValueError, match="fills"):
            groups.GroupSuccessiveHalving([3, 1], [1, 3], fills=bad)
    with pytest.raises(ValueError, match="fills"):
        groups.GroupHyperband(None, fills="most")
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="skip_random"):
            groups.GroupBOHB(2, "cc", [0, 0], skip_random=bad)
