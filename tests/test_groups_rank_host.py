"""Grouped log-ratio ranking, host side (no GPU): the C ABI's argument handling, the size helpers, the Python checks."""
import numpy as np
import pytest

P = 4096  # a non-null, 16-byte aligned placeholder: every check precedes the first launch, nothing is dereferenced


def _rank(L, ll=P, lg=P, status=P, B=3, C=100, k=8, res=P, ws=P, wsb=1 << 20):
    return L.hbx_kde_rank_groups(ll, lg, status, B, C, k, res, ws, wsb, None)


def _composite(L, B=3, C=100, k=8, D=4, res=P, ws=P, wsb=1 << 30, cand=P):
    return L.hbx_kde_rank_logratio_groups(P, D, P, B, P, P, P, P, P, P, P, P, cand, C, k, 1e-5, 1, res, ws, wsb, None)


@pytest.mark.parametrize("call,name", [(_rank, b"hbx_kde_rank_groups:"), (_composite, b"hbx_kde_rank_logratio_groups:")])
@pytest.mark.parametrize("kw,word", [(dict(res=None), b"null"), (dict(ws=None), b"null"), (dict(k=0), b"k=0"),
                                     (dict(k=1025, C=2000), b"k=1025"), (dict(k=9, C=8), b"exceeds C=8"),
                                     (dict(B=-1), b"B=-1"), (dict(wsb=8), b"workspace too small"),
                                     (dict(B=1 << 20, C=1 << 12), b"int32")])
def test_bad_arguments_are_refused_before_any_launch(call, name, kw, word):
    from hpbandster_amd import _native as N
    L = N.lib()
    assert call(L, **kw) in (-1, -3)
    msg = L.hbx_last_error()
    assert name in msg and word in msg, msg


def test_rank_alone_null_inputs_and_nothing_to_do():
    from hpbandster_amd import _native as N
    L = N.lib()
    for kw in (dict(ll=None), dict(lg=None), dict(status=None)):
        assert _rank(L, **kw) == -1 and b"hbx_kde_rank_groups: null" in L.hbx_last_error()
    assert _rank(L, ll=P + 4) == -1 and b"aligned" in L.hbx_last_error()
    assert _composite(L, cand=None) == -1 and b"hbx_kde_logpdf_groups: null" in L.hbx_last_error()  # (its own check)
    assert _rank(L, B=0) == 0 and _composite(L, B=0) == 0  # nothing launched


def test_size_helpers():
    from hpbandster_amd import _native as N
    L = N.lib()
    f, g = L.hbx_kde_rank_groups_workspace_bytes, L.hbx_kde_rank_logratio_groups_workspace_bytes
    assert f(10000, 64, 16) > 0 and f(0, 64, 16) > 0 and f(3, 1, 1) > 0
    assert f(64, 100000, 130) >= 64 * (100000 // 16384) * 130 * 4  # a sliced pool: k indices per slice
    assert f(3, 2000, 1025) < 0 and f(3, 100, 0) < 0 and f(3, 7, 8) < 0 and f(-1, 64, 8) < 0
    assert f(1 << 20, 1 << 12, 8) < 0
    lp = L.hbx_kde_logpdf_groups_workspace_bytes(100, 64, 32)
    assert g(100, 64, 8, 32) >= lp + 2 * 100 * 64 * 8 + 100 * 4 + f(100, 64, 8)
    assert g(100, 64, 1025, 32) < 0 and g(100, 64, 8, 0) < 0


def test_python_checks_and_blocks():
    from hpbandster_amd import groups
    gm = groups.GroupModel(B=2, D=3, device=None)
    with pytest.raises(ValueError):
        gm.propose(4, 0, [0, 0, 0], topk=2, score="bogus")
    with pytest.raises(ValueError):
        groups.rank_values(np.zeros((2, 5)), np.zeros((2, 4)), 2)
    with pytest.raises(ValueError):
        groups.rank_values(np.zeros((2, 5)), np.zeros((2, 5)), 2, status=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        groups.rank_values(np.zeros((2, 5)), np.zeros((2, 5)), 6)
    k = 2
    raw = np.zeros((2, groups.RANK_HEAD_BYTES + k * groups.RANK_REC.itemsize), dtype=np.uint8)
    assert raw.shape[1] == 16 + 32 * k
    raw[:, :16].view("<i4")[:] = [[1, k, 0, 0], [0, k, groups.ACQ_NO_MODEL, 0]]
    rec = raw[:, 16:].view(groups.RANK_REC)
    rec[:] = (-1, 0, np.nan, np.nan, np.nan)
    rec[0, 0] = (4, 0, -1.5, -20.0, -21.5)
    r = groups.GroupRank.from_bytes(raw.tobytes(), 2, k)
    assert len(r) == 2 and list(r.count) == [1, 0] and list(r.status) == [0, groups.ACQ_NO_MODEL]
    assert r.index.tolist() == [[4, -1], [-1, -1]] and r.top(0)[1].tolist() == [-1.5] and r.top(1)[0].size == 0
    cands = np.arange(2 * 6 * 3, dtype=np.float64).reshape(2, 6, 3)
    rows = r.rows(cands)
    np.testing.assert_array_equal(rows[0, 0], cands[0, 4])
    assert np.all(np.isnan(rows[0, 1])) and np.all(np.isnan(rows[1])) and "GroupRank" in repr(r)
