"""distributed.merge_topk (host only): per-shard top-k results with global indices merged into the global top-k
by (score, index) -- what KDEPair.acquire_topk returns over the whole pool.  Also host only: the result block's
decoding and the C entry points' size helpers and argument checks."""
import numpy as np
import pytest

from hpbandster_amd.distributed import merge_topk
from hpbandster_amd.kde import ACQ_NEAR_TIE, ACQ_OVERFLOW, TopK


def _part(index, score, shortlist=0, flags=0):
    index = np.asarray(index, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    # pdfs and bounds that identify their entry: pdf_l = index + 0.5, pdf_g = score * pdf_l, rel = index * 2^-40
    return TopK(index, score, index + 0.5, score * (index + 0.5), (index * 2.0 ** -40).astype(np.float32),
                shortlist, flags)


def _rows(t):
    return list(zip(t.index.tolist(), t.score.tolist(), t.pdf_l.tolist(), t.pdf_g.tolist(), t.rel.tolist()))


def test_merge_is_the_sort_of_all_entries():
    rs = np.random.RandomState(0)
    parts, allr = [], []
    for r in range(5):
        n = int(rs.randint(0, 9))
        idx = np.sort(rs.choice(100, n, replace=False)) + 100 * r
        sc = np.sort(np.round(rs.rand(n) * 4) / 4)  # many equal scores
        o = np.lexsort((idx, sc))
        parts.append(_part(idx[o], sc[o], shortlist=n + 1))
        allr += _rows(parts[-1])
    allr.sort(key=lambda e: (e[1], e[0]))
    for k in (1, 3, 10, 1024):
        m = merge_topk(parts, k)
        assert m.count == min(k, len(allr)) == len(m.index)
        assert _rows(m) == allr[:k]
        assert m.shortlist == sum(p.shortlist for p in parts)
        assert m.index.dtype == np.int64 and m.score.dtype == np.float64 and m.rel.dtype == np.float32


def test_ties_across_shards_go_to_the_smaller_global_index():
    a = _part([7, 9], [0.5, 0.5])
    b = _part([1003, 1004], [0.25, 0.5])
    c = _part([2], [0.5])
    m = merge_topk([b, a, c], 4)  # whatever order the parts arrive in
    assert m.index.tolist() == [1003, 2, 7, 9]
    assert m.score.tolist() == [0.25, 0.5, 0.5, 0.5]
    assert _rows(m)[1] == _rows(c)[0]
    assert merge_topk([a, b, c], 2).index.tolist() == [1003, 2]


def test_short_and_empty_parts():
    a = _part([5], [2.0], shortlist=3, flags=ACQ_NEAR_TIE)
    e = _part([], [], shortlist=0, flags=ACQ_OVERFLOW)
    m = merge_topk([e, a, e], 8)  # fewer than k in all
    assert m.count == 1 and m.index.tolist() == [5] and m.flags == ACQ_NEAR_TIE | ACQ_OVERFLOW and m.shortlist == 3
    z = merge_topk([e, e], 4)
    assert z.count == 0 and z.index.size == 0 and z.score.size == 0 and z.rel.size == 0
    assert merge_topk([], 4).count == 0
    with pytest.raises(ValueError):
        merge_topk([a], 0)
    with pytest.raises(ValueError):
        merge_topk([a], 1025)


def test_result_block_round_trip():
    """TopK.from_bytes reads the documented block: a 16-byte header, then 40-byte records."""
    import struct
    blob = struct.pack("<iiii", 2, 9, ACQ_NEAR_TIE, 4)
    blob += struct.pack("<qdddfi", 11, 0.5, 2.0, 1.0, 2.0 ** -45, 0) + struct.pack("<qdddfi", 3, 0.75, 4.0, 3.0, 0.0, 0)
    blob += b"\xff" * 80  # the unwritten records of a k = 4 block
    t = TopK.from_bytes(blob)
    assert (t.count, t.shortlist, t.flags) == (2, 9, ACQ_NEAR_TIE)
    assert _rows(t) == [(11, 0.5, 2.0, 1.0, 2.0 ** -45), (3, 0.75, 4.0, 3.0, 0.0)]


def test_c_abi_sizes_and_bad_arguments():
    """The size helpers and hbx_kde_acquire_topk's argument checks (they return before anything is launched)."""
    from hpbandster_amd import _native as N
    L = N.lib()
    assert L.hbx_kde_topk_result_bytes(1) == 56 and L.hbx_kde_topk_result_bytes(1024) == 16 + 40 * 1024
    assert L.hbx_kde_topk_result_bytes(0) == -1 and L.hbx_kde_topk_result_bytes(1025) == -1
    base = L.hbx_kde_workspace_bytes(700, 1000)
    assert L.hbx_kde_topk_workspace_bytes(700, 64, 1000) == base + 4096
    assert L.hbx_kde_topk_workspace_bytes(700, 0, 1000) == -1
    buf = np.zeros(64)
    p = N.ptr(buf)  # a valid host address: the checks below return before any pointer is used
    pair = L.hbx_kde_pair_bind(8, p, p, p, p, 0, p, p, p, p, 0, 8, 0, 1000)  # a pair over the dummy address
    assert pair
    try:
        for k in (0, 1025):
            assert L.hbx_kde_acquire_topk(p, 8, k, 0, pair, p, p, 1 << 30, None) != 0
            assert b"k=" in L.hbx_last_error()
        assert L.hbx_kde_acquire_topk(p, 8, 4, 0, pair, None, p, 1 << 30, None) != 0  # no result buffer
        assert b"null" in L.hbx_last_error()
        assert L.hbx_kde_acquire_topk(p, 8, 4, 0, pair, p, p, 16, None) != 0  # workspace too small
        assert b"workspace" in L.hbx_last_error()
    finally:
        L.hbx_kde_pair_free(pair)
