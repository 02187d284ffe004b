"""Grouped acquisition with S requests per group, host side (no GPU): GroupPicks over a [B, S] record buffer and the
new entry points' argument handling."""
import numpy as np
import pytest


def _records(B, S, C, seed=0):
    """B * S hand-made records in request order b * S + s; every third one has no pick"""
    from hpbandster_amd import groups
    rs = np.random.RandomState(seed)
    r = np.zeros(B * S, dtype=groups.RECORD)
    r["index"] = rs.randint(0, C, size=B * S)
    r["score"] = rs.rand(B * S)
    r["pdf_l"] = rs.rand(B * S)
    r["pdf_g"] = rs.rand(B * S)
    r["rel"] = 1e-14
    r["flags"] = rs.randint(0, 4, size=B * S)
    r["shortlist"] = rs.randint(1, C + 1, size=B * S)
    r["near"] = 1
    none = np.arange(B * S) % 3 == 1
    r["index"][none] = -1
    r["score"][none] = np.nan
    return r


def test_picks_of_shape_b_s():
    from hpbandster_amd import groups
    B, S, C, D = 4, 3, 5, 2
    r = _records(B, S, C)
    p = groups.GroupPicks.from_bytes(r.tobytes(), B, S)
    assert len(p) == B
    for name in groups.GroupPicks.__slots__:
        a = getattr(p, name)
        assert a.shape == (B, S) and a.flags["C_CONTIGUOUS"], name
        np.testing.assert_array_equal(a.reshape(-1), r[name])  # record b * S + s is element [b, s]
    assert p.index[2, 1] == r["index"][2 * S + 1] and p.shortlist.dtype == np.int32 and p.rel.dtype == np.float32
    cands = np.random.RandomState(1).rand(B, S, C, D)
    rows = p.rows(cands)
    assert rows.shape == (B, S, D)
    for b in range(B):
        for s in range(S):
            if p.index[b, s] < 0:
                assert np.isnan(rows[b, s]).all()
            else:
                np.testing.assert_array_equal(rows[b, s], cands[b, s, p.index[b, s]])
    with pytest.raises(Exception):
        p.rows(cands[:, 0])  # a [B, C, D] pool does not belong to [B, S] picks
    assert "S=3" in repr(p)
    e = groups.GroupPicks.from_bytes(b"", 0, 3)
    assert len(e) == 0 and e.index.shape == (0, 3) and e.rows(np.empty((0, 3, C, D))).shape == (0, 3, D)
    z = groups.GroupPicks.from_bytes(b"", 4, 0)
    assert len(z) == 4 and z.index.shape == (4, 0) and z.rows(np.empty((4, 0, C, D))).shape == (4, 0, D)


def test_the_one_dimensional_form_is_unchanged():
    from hpbandster_amd import groups
    B, C, D = 6, 5, 3
    r = _records(B, 1, C, seed=2)
    p = groups.GroupPicks.from_bytes(r.tobytes(), B)
    q = groups.GroupPicks(r)
    assert len(p) == B and p.index.shape == (B,)
    for name in groups.GroupPicks.__slots__:
        np.testing.assert_array_equal(getattr(p, name), r[name])
        np.testing.assert_array_equal(getattr(q, name), r[name])
    cands = np.random.RandomState(3).rand(B, C, D)
    rows = p.rows(cands)
    assert rows.shape == (B, D)
    for b in range(B):
        if p.index[b] < 0:
            assert np.isnan(rows[b]).all()
        else:
            np.testing.assert_array_equal(rows[b], cands[b, p.index[b]])
    assert repr(p).startswith("GroupPicks(B=6, picked=")


def test_batch_entry_points_check_their_arguments():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name in ("hbx_kde_groups_batch_workspace_bytes", "hbx_kde_acquire_groups_batch"):
        assert hasattr(L, name) and name in N.SIGNATURES, name
    f = L.hbx_kde_groups_batch_workspace_bytes
    assert f(10, 1, 64, 32) == L.hbx_kde_groups_workspace_bytes(10, 64, 32)
    assert f(10, 4, 64, 32) == 256 + 10 * 4 * 64 * 16
    assert f(0, 4, 64, 32) > 0 and f(10, 0, 64, 32) > 0 and f(10, 4, 0, 32) > 0  # zero-safe
    assert f(-1, 1, 1, 1) < 0 and f(1, -1, 1, 1) < 0 and f(1, 1, -1, 1) < 0 and f(1, 1, 1, 0) < 0 and f(1, 1, 1, 257) < 0
    assert f(1 << 12, 1 << 10, 1 << 10, 32) == -1 and f(1 << 20, 1 << 12, 1, 32) == -1  # B * S * C past int32
    assert f(1 << 10, 1 << 10, 1 << 10, 32) > 0  # 2^30: inside

    def acq(B=4, S=3, C=8, D=3, X=4096, res=4096, ws=4096, wsb=1 << 20):
        p = 4096  # non-null placeholders are never dereferenced: every check precedes the launches
        return L.hbx_kde_acquire_groups_batch(X or None, D, p, B, p, p, p, p, p, p, p, p, p, S, C, res or None,
                                              ws or None, wsb, None)

    assert acq(X=0) == -1 and b"hbx_kde_acquire_groups_batch" in L.hbx_last_error() and b"null" in L.hbx_last_error()
    assert acq(res=0) == -1 and acq(ws=0) == -1
    assert acq(S=-1) == -1 and b"S=-1" in L.hbx_last_error()
    assert acq(B=-1) == -1 and acq(C=-3) == -1 and acq(D=0) == -1 and acq(D=257) == -1
    assert acq(B=1 << 12, S=1 << 10, C=1 << 10) == -1 and b"int32" in L.hbx_last_error()
    assert acq(wsb=256 + 4 * 3 * 8 * 16 - 1) == -1 and b"workspace too small" in L.hbx_last_error()
    assert acq(ws=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert acq(B=0) == 0 and acq(S=0) == 0  # nothing to do, nothing launched
