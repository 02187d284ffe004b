"""Single-pool top-k by log ratio (hbx_kde_acquire_topk_lr; KDEPair.acquire_topk(score="log_ratio")) on the GPU against tests/test_gpu_acquire_lr.py's reference: the oracle's exact
pdfs, its log-space value where a pdf underflowed, a tolerance per candidate.  The reference ranking is the non-NaN s
by (s, index).  Every case is decided (asserted first): each adjacent pair among the reference's first count + 1
entries lies further apart than both tolerances, exact duplicates excepted (checked on the host with the C oracle:
the pools' seed 0 serves every case).

Candidate counts: 5 (k > F); 130; 4100 past one 4096-key histogram block and EXACT_SCAN_MAX; 70 000 an unsplit scoring
launch.  k = 1024 merges past one chunk of the ranking block; k = 64 on `under` ranks the 47 far candidates' log-space
values among the others (this pool has no infinite s)."""
import numpy as np
import pytest

from tests import test_gpu_acquire_lr as A

pytestmark = pytest.mark.gpu

NEAR_TIE, OVERFLOW, LOG_RATIO = 2, 1, 128
CASES = [(kind, C, k) for kind in sorted(A.KINDS) for C in (5, 130, 4100, 70000) for k in ((8,) if C == 5 else (1, 8))]
CASES += [("c3u2", 4100, 1024), ("under", 130, 64)]


def _ranking(s, tol, k):
    """the reference's first min(k, F) indices by (s, index), NaN never; asserts that the case is decided"""
    ok = np.flatnonzero(~np.isnan(s))
    order = ok[np.lexsort((ok, s[ok]))]
    for a, b in zip(order[:k], order[1:k + 1]):
        assert s[a] == s[b] or s[b] - s[a] > tol[a] + tol[b], (a, b, s[a], s[b])
    return order[:k]


def _check(top, want, s, tol, pl, pg, tag):
    print(tag, "count", top.count, "shortlist", top.shortlist, "flags", top.flags, "index", top.index[:8])
    assert top.count == len(want) and list(top.index) == list(want) and 1 not in top.index, tag
    assert top.pdf_l.tobytes() == pl[want].tobytes() and top.pdf_g.tobytes() == pg[want].tobytes(), tag
    with np.errstate(invalid="ignore"):
        assert np.all((top.score == s[want]) | (np.abs(top.score - s[want]) <= tol[want])), tag
    assert top.flags & LOG_RATIO, tag


@pytest.mark.parametrize("kind,C,k", CASES)
def test_ranking_equals_the_reference(device, kind, C, k):
    pair, pool, s, tol, pl, pg, under = A._case(device, kind, C)
    want = _ranking(s, tol, k)
    top = pair.acquire_topk(pool, k, score="log_ratio")
    _check(top, want, s, tol, pl, pg, (kind, C, k))
    assert top.count == min(k, int(np.sum(~np.isnan(s)))) and bool(top.flags & OVERFLOW) == (kind == "exact")
    assert k != 64 or np.sum(under[want]) >= 40  # log-space values inside the ranking


@pytest.mark.parametrize("kind", ["c3u2", "under"])
def test_entry_0_is_the_single_pick(device, kind):
    """on `under` the winner's L is a log-space value"""
    pair, pool, s, tol, pl, pg, under = A._case(device, kind, 130)
    top, r = pair.acquire_topk(pool, 8, score="log_ratio"), pair.acquire(pool, score="log_ratio")
    assert kind != "under" or under[r.index]
    assert (top.index[0], top.score[0].tobytes(), top.pdf_l[0].tobytes(), top.pdf_g[0].tobytes()) == \
        (r.index, np.float64(r.score).tobytes(), np.float64(r.pdf_l).tobytes(), np.float64(r.pdf_g).tobytes())


def test_ties_come_in_index_order(device):
    pair, pool, s, tol, *_ = A._case(device, "c3u2", 130)
    win = int(_ranking(s, tol, 1)[0])
    assert win < 100
    tied = pool.copy()
    tied[[100, 129]] = pool[win]
    top = pair.acquire_topk(tied, 3, score="log_ratio")
    assert list(top.index) == [win, 100, 129] and top.score[0] == top.score[1] == top.score[2]


def test_no_score_and_empty_pool(device):
    pair, pool, *_ = A._case(device, "c3u2", 130)
    for cands in (np.full_like(pool, np.nan), pool[:0]):
        assert pair.acquire_topk(cands, 8, score="log_ratio").count == 0


def test_shards_merge_to_the_one_pool_call(device):
    from hpbandster_amd.distributed import merge_topk
    pair, pool, *_ = A._case(device, "c3u2", 130)
    whole = pair.acquire_topk(pool, 8, score="log_ratio")
    parts = [pair.acquire_topk(pool[a:b], 8, index_base=a, score="log_ratio") for a, b in ((0, 65), (65, 130))]
    merged = merge_topk(parts, 8)
    assert merged.count == whole.count == 8 and merged.flags == whole.flags
    for f in ("index", "score", "pdf_l", "pdf_g", "rel"):
        assert getattr(merged, f).tobytes() == getattr(whole, f).tobytes(), f


def test_the_floored_ranking_is_the_lowest_indices_where_the_log_ratio_decides(device):
    """test_the_floored_score_ties_where_the_log_ratio_decides' model and pool: every floored score is exactly 1"""
    pair, vt, kdes = A._model(device, "signed")
    rs = np.random.RandomState(0)
    pool = np.concatenate((3 * rs.rand(256, 24) - 1, rs.randint(0, 4, size=(256, 8))), axis=1).astype(np.float64)
    pool[1, 0] = np.nan
    s, tol, pl, pg, _ = A._reference(kdes, vt, pool)
    want = _ranking(s, tol, 8)
    floored = pair.acquire_topk(pool, 8)
    assert list(floored.index) == [0, 2, 3, 4, 5, 6, 7, 8] and np.all(floored.score == 1.0)
    assert list(want) != list(floored.index)
    _check(pair.acquire_topk(pool, 8, score="log_ratio"), want, s, tol, pl, pg, "signed/rand")
