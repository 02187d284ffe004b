"""Grouped ln-pdf, host side (no GPU): the C ABI's argument handling, the workspace size and GroupLogPdf's shapes."""
import numpy as np
import pytest

NEW = ["hbx_kde_logpdf_groups_workspace_bytes", "hbx_kde_logpdf_groups", "hbx_kde_logpdf_groups_stats"]


def test_symbols_exported_and_bound():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES, name


def test_workspace_bytes():
    from hpbandster_amd import _native as N
    f = N.lib().hbx_kde_logpdf_groups_workspace_bytes
    assert f(1, 1, 1) > 0
    assert f(0, 64, 32) > 0 and f(10, 0, 32) > 0  # zero-safe
    prev = 0
    for B in (1, 2, 7, 1000, 10000):
        v = f(B, 64, 32)
        assert v > prev
        prev = v
    prev = 0
    for C in (1, 2, 64, 65, 300, 4096):
        v = f(100, C, 32)
        assert v > prev
        prev = v
    # a list segment of C entries per (group, KDE): a list can never overflow
    assert f(10000, 64, 32) >= 10000 * 64 * 2 * 4
    # out of range: negative sizes, D, B * C past int32
    assert f(-1, 64, 32) == -1 and f(1, -1, 32) == -1 and f(1, 1, 0) == -1 and f(1, 1, 257) == -1
    assert f(1 << 20, 1 << 12, 32) == -1


def test_bad_arguments_are_errors():
    from hpbandster_amd import _native as N
    L = N.lib()
    p = 4096  # non-null placeholders are never dereferenced: every check precedes the first launch

    def call(B=4, C=8, D=3, X=p, cand=p, rtol=1e-5, flags=0, ll=p, lg=p, status=p, ws=p, wsb=1 << 20):
        return L.hbx_kde_logpdf_groups(X, D, p, B, p, p, p, p, p, p, p, p, cand, C, rtol, flags, ll, lg, status, ws,
                                       wsb, None)

    def failed(rc, *words):
        msg = L.hbx_last_error()
        return rc == -1 and b"hbx_kde_logpdf_groups" in msg and all(w in msg for w in words)

    assert failed(call(X=None), b"null")
    assert failed(call(cand=None), b"null")
    assert failed(call(status=None), b"null")
    assert failed(call(ws=None), b"null")
    assert failed(call(ll=None, lg=None), b"null")  # both outputs NULL
    assert failed(call(B=-1), b"B=-1")
    assert failed(call(C=-3), b"C=-3")
    assert failed(call(D=0), b"D=0") and failed(call(D=257), b"D=257")
    assert failed(call(rtol=0.0), b"rtol") and failed(call(rtol=-1.0), b"rtol") and failed(call(rtol=float("nan")), b"rtol")
    assert failed(call(flags=2), b"flags")
    assert failed(call(B=1 << 20, C=1 << 12), b"int32")
    assert failed(call(wsb=16), b"workspace too small")
    need = L.hbx_kde_logpdf_groups_workspace_bytes(4, 8, 3)
    assert failed(call(wsb=need - 1), b"workspace too small")
    assert failed(call(ws=4104), b"aligned")
    assert failed(call(ll=4100), b"aligned")
    assert failed(call(cand=4097), b"aligned")
    assert failed(call(status=4098), b"aligned")
    # nothing to do, nothing launched (and nothing dereferenced): B == 0, C == 0
    assert call(B=0) == 0
    assert call(C=0) == 0
    assert call(B=0, ll=None) == 0  # one output is enough
    # the stats reader checks its pointers too
    assert L.hbx_kde_logpdf_groups_stats(None, None) == -1 and b"hbx_kde_logpdf_groups_stats" in L.hbx_last_error()


def test_group_logpdf_shapes():
    from hpbandster_amd import groups
    B, S, C = 3, 2, 5
    ll = np.arange(B * S * C, dtype=np.float64).reshape(B, S * C)
    lg = -ll
    st = np.array([0, groups.ACQ_NO_MODEL, groups.GRP_EXACT_L | groups.GRP_EXACT_G], dtype=np.int32)
    r = groups.GroupLogPdf(ll, lg, st, [1, 2, 3, 4], (B, S * C))
    assert len(r) == B and r.ln_l.shape == (B, S * C) and r.ln_g.shape == (B, S * C)
    assert r.ln_l.dtype == np.float64 and r.status.dtype == np.int32 and r.stats == (1, 2, 3, 4)
    r4 = groups.GroupLogPdf(ll, lg, st, [1, 2, 3, 4], (B, S, C))
    assert r4.ln_l.shape == (B, S, C) and r4.ln_g.shape == (B, S, C)
    np.testing.assert_array_equal(r4.ln_l.reshape(B, S * C), ll)  # request (b, s) is the flattened pool's slice
    np.testing.assert_array_equal(r4.ln_l[1, 1], ll[1, C:])
    one = groups.GroupLogPdf(ll, None, st, None, (B, S, C))
    assert one.ln_g is None and one.stats is None and one.ln_l.shape == (B, S, C)
    e = groups.GroupLogPdf(np.empty((0, 0)), np.empty((0, 0)), np.empty(0, np.int32), [0, 0, 0, 0], (0, 0))
    assert len(e) == 0 and e.ln_l.shape == (0, 0)
    assert (groups.GRP_EXACT_L, groups.GRP_EXACT_G, groups.LOGPDF_FP64_ONLY) == (64, 128, 1)
    assert "GroupLogPdf" in repr(r)


def test_logpdf_rejects_bad_python_arguments():
    from hpbandster_amd import groups
    gm = groups.GroupModel(B=2, D=3, device=None)
    with pytest.raises(ValueError):
        gm.logpdf(np.zeros((2, 4, 3)), which="neither")
    with pytest.raises(ValueError):
        gm.logpdf(np.zeros((2, 4, 3)), rtol=0.0)
