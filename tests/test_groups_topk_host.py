"""Grouped top-k, host side (no GPU): the C ABI's argument handling, the workspace size and GroupTopK's parsing."""
import struct

import numpy as np
import pytest

NEW = ["hbx_kde_groups_topk_workspace_bytes", "hbx_kde_acquire_groups_topk"]


def test_symbols_exported_and_bound():
    from hpbandster_amd import _native as N
    L = N.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES, name


def test_workspace_bytes():
    from hpbandster_amd import _native as N
    f = N.lib().hbx_kde_groups_topk_workspace_bytes
    g = N.lib().hbx_kde_groups_workspace_bytes
    assert f(1, 1, 1, 1) > 0
    assert f(0, 64, 4, 32) > 0 and f(10, 0, 4, 32) > 0  # zero-safe
    prev = 0
    for B in (1, 2, 7, 1000, 10000):
        v = f(B, 64, 16, 32)
        assert v > prev and v >= g(B, 64, 32)
        prev = v
    prev = 0
    for C in (1, 2, 64, 65, 300, 4096):
        v = f(100, C, 16, 32)
        assert v > prev and v >= g(100, C, 32)
        prev = v
    prev = 0
    for k in (1, 2, 16, 255, 256, 767, 768, 1024):  # never shrinks with k
        v = f(100, 2500, k, 32)
        assert v >= prev and v >= g(100, 2500, 32)
        prev = v
    # the re-scored candidates' pdfs: 16 bytes each behind the screen's 16
    assert f(10000, 64, 4, 32) >= 10000 * 64 * 32
    # out of range: k, negative sizes, D, B * C past int32
    assert f(4, 64, 0, 32) == -1 and f(4, 64, 1025, 32) == -1 and f(4, 64, -1, 32) == -1
    assert f(-1, 64, 4, 32) == -1 and f(1, -1, 4, 32) == -1 and f(1, 1, 4, 0) == -1 and f(1, 1, 4, 257) == -1
    assert f(1 << 20, 1 << 12, 4, 32) == -1


def test_bad_arguments_are_errors():
    from hpbandster_amd import _native as N
    L = N.lib()

    def acq(B=4, C=8, D=3, k=2, X=1, res=4096, ws=4096, wsb=1 << 20):
        # non-null placeholders are never dereferenced: every check precedes the launch
        p = 4096
        return L.hbx_kde_acquire_groups_topk(p if X else None, D, p, B, p, p, p, p, p, p, p, p, p, C, k, res, ws, wsb,
                                             None)

    assert acq(X=0) == -1 and b"hbx_kde_acquire_groups_topk" in L.hbx_last_error() and b"null" in L.hbx_last_error()
    assert acq(res=None) == -1 and b"null" in L.hbx_last_error()
    assert acq(ws=None) == -1
    assert acq(B=-1) == -1 and b"B=-1" in L.hbx_last_error()
    assert acq(C=-3) == -1
    assert acq(D=0) == -1 and acq(D=257) == -1
    assert acq(k=0) == -1 and b"k=0" in L.hbx_last_error()
    assert acq(k=1025) == -1 and b"k=1025" in L.hbx_last_error()
    assert acq(B=1 << 20, C=1 << 12) == -1 and b"int32" in L.hbx_last_error()
    assert acq(wsb=16) == -1 and b"workspace too small" in L.hbx_last_error()
    need = L.hbx_kde_groups_topk_workspace_bytes(4, 8, 2, 3)
    assert acq(wsb=need - 1) == -1 and b"workspace too small" in L.hbx_last_error()
    assert acq(wsb=L.hbx_kde_groups_workspace_bytes(4, 8, 3)) == -1  # the grouped call's size is not enough
    assert acq(ws=4104) == -1 and b"aligned" in L.hbx_last_error()
    assert acq(res=4100) == -1 and b"aligned" in L.hbx_last_error()
    assert acq(B=0) == 0  # nothing to do, nothing launched


def _block(k, count, shortlist, flags, recs, fill=0xAB):
    """One result block by hand: the header, `count` records, then unspecified bytes."""
    from hpbandster_amd import kde
    b = struct.pack("<iiii", count, shortlist, flags, k)
    for (i, s, l, g, r) in recs:
        b += struct.pack("<qdddfi", i, s, l, g, r, 0)
    return b + bytes([fill]) * (kde.TOPK_HEAD_BYTES + kde.TOPK_REC.itemsize * k - len(b))


def test_group_topk_from_bytes_top_and_rows():
    from hpbandster_amd import groups, kde
    k, B = 3, 4
    recs = {0: [(5, 0.25, 2.0, 0.5, 1e-14), (1, 0.5, 1.0, 0.5, 2e-14), (7, 0.5, 3.0, 1.5, 3e-14)],  # full
            1: [(2, 1.0, 1e-9, 1e-9, 1e-14)],                                                        # ragged
            2: [], 3: []}                                                                          # empty
    heads = {0: (3, 6, 0), 1: (1, 1, kde.ACQ_NEAR_TIE), 2: (0, 0, groups.ACQ_NO_MODEL), 3: (0, 8, kde.ACQ_OVERFLOW)}
    raw = b"".join(_block(k, heads[b][0], heads[b][1], heads[b][2], recs[b]) for b in range(B))
    assert len(raw) == B * (16 + 40 * k)
    t = groups.GroupTopK.from_bytes(raw, B, k)
    assert len(t) == B and t.k == k
    for name, dt, shape in (("count", np.int32, (B,)), ("shortlist", np.int32, (B,)), ("flags", np.int32, (B,)),
                            ("index", np.int64, (B, k)), ("score", np.float64, (B, k)),
                            ("pdf_l", np.float64, (B, k)), ("pdf_g", np.float64, (B, k)), ("rel", np.float32, (B, k))):
        a = getattr(t, name)
        assert a.dtype == dt and a.shape == shape, name
    np.testing.assert_array_equal(t.count, [3, 1, 0, 0])
    np.testing.assert_array_equal(t.shortlist, [6, 1, 0, 8])
    np.testing.assert_array_equal(t.flags, [0, kde.ACQ_NEAR_TIE, groups.ACQ_NO_MODEL, kde.ACQ_OVERFLOW])
    np.testing.assert_array_equal(t.index, [[5, 1, 7], [2, -1, -1], [-1, -1, -1], [-1, -1, -1]])
    np.testing.assert_array_equal(t.score[0], [0.25, 0.5, 0.5])
    np.testing.assert_array_equal(t.pdf_l[0], [2.0, 1.0, 3.0])
    np.testing.assert_array_equal(t.pdf_g[0], [0.5, 0.5, 1.5])
    np.testing.assert_array_equal(t.rel[0], np.array([1e-14, 2e-14, 3e-14], dtype=np.float32))
    assert t.score[1, 0] == 1.0 and np.all(np.isnan(t.score[1, 1:]))
    for name in ("score", "pdf_l", "pdf_g"):  # the unspecified bytes past count are never read
        assert np.all(np.isnan(getattr(t, name)[2:])), name
    # top(b): the group as the single path's TopK
    t0 = t.top(0)
    assert isinstance(t0, kde.TopK) and t0.count == 3 and t0.shortlist == 6 and t0.flags == 0
    np.testing.assert_array_equal(t0.index, [5, 1, 7])
    np.testing.assert_array_equal(t0.pdf_g, [0.5, 0.5, 1.5])
    t1 = t.top(1)
    assert t1.count == 1 and t1.flags == kde.ACQ_NEAR_TIE and t1.index.tolist() == [2] and t1.rel.shape == (1,)
    assert t.top(2).count == 0 and t.top(2).flags == groups.ACQ_NO_MODEL and t.top(3).shortlist == 8
    # rows on a numpy pool
    C, D = 9, 2
    cands = np.arange(B * C * D, dtype=np.float64).reshape(B, C, D)
    rows = t.rows(cands)
    assert rows.shape == (B, k, D)
    np.testing.assert_array_equal(rows[0], cands[0, [5, 1, 7]])
    np.testing.assert_array_equal(rows[1, 0], cands[1, 2])
    assert np.all(np.isnan(rows[1, 1:])) and np.all(np.isnan(rows[2:]))
    with pytest.raises(Exception):
        t.rows(cands[:2])
    # a count past k is not a block this call wrote
    with pytest.raises(Exception):
        groups.GroupTopK.from_bytes(_block(k, k + 1, 0, 0, []), 1, k)
    # B = 0
    e = groups.GroupTopK.from_bytes(b"", 0, k)
    assert len(e) == 0 and e.index.shape == (0, k) and e.rows(np.empty((0, C, D))).shape == (0, k, D)
