"""Grouped top-k (hbx_kde_acquire_groups_topk, GroupModel.acquire_topk) on the GPU: per group the first min(k, F)
entries of the stable ascending order of the oracle's non-NaN scores (c_oracle.kde_pdf(exact=True) + py_score), index,
score and both pdfs bit for bit; entry 0 the grouped pick's; the single path's top-k for the same pair.  Pools and
oracle are tests/test_gpu_groups.py's construction (24 ragged groups with its deliberate ones).
"""
import numpy as np
import pytest

from oracle import kde_oracle as O
from tests.test_gpu_groups import NEAR_TIE, NO_MODEL, OVERFLOW, UNSUPPORTED, _groups, _oracle, _same

pytestmark = pytest.mark.gpu

SHAPES = [(1, 0), (0, 3), (5, 2), (24, 8)]
_cache = {}


def _ranked(l, g):
    """(scores, order): py_score per candidate and the stable ascending order of the non-NaN ones."""
    s = np.array([O.py_score(float(a), float(b)) for a, b in zip(l, g)], dtype=np.float64)
    ok = np.nonzero(~np.isnan(s))[0]
    return s, ok[np.argsort(s[ok], kind="stable")]


def _case(device, dc, du, C):
    """The fitted model, the pools and the oracle of every group with a model, computed once per (shape, C) and
    never changed (tests that edit a pool copy it)."""
    key = (dc, du, C)
    if key not in _cache:
        from hpbandster_amd import groups
        X, losses, seg, vt, levels, cands, kinds = _groups(dc, du, C)
        gm = groups.fit_groups(X, losses, seg, vt, device=device)
        ora = {}
        for b in range(gm.B):
            if kinds.get(b) in ("no_model", "unsupported"):
                continue
            l, g = _oracle(gm, X, seg, vt, cands, b)
            ora[b] = (l, g) + _ranked(l, g)
        _cache[key] = (gm, X, seg, vt, cands, kinds, ora)
    return _cache[key]


def _check_block(top, b, ora, k, tag=None):
    """Block b of a GroupTopK against the oracle (l, g, s, order)."""
    l, g, s, order = ora
    want = order[:k]
    tag = (tag, b, k)
    assert top.count[b] == len(want), (tag, top.count[b], len(want))
    c = len(want)
    np.testing.assert_array_equal(top.index[b, :c], want, err_msg=str(tag))
    np.testing.assert_array_equal(top.index[b, c:], -1, err_msg=str(tag))
    np.testing.assert_array_equal(top.score[b, :c].view(np.int64), s[want].view(np.int64), err_msg=str(tag))
    np.testing.assert_array_equal(top.pdf_l[b, :c], l[want], err_msg=str(tag))
    np.testing.assert_array_equal(top.pdf_g[b, :c], g[want], err_msg=str(tag))
    assert np.all(np.isnan(top.score[b, c:])) and top.shortlist[b] >= top.count[b], tag


@pytest.mark.parametrize("k", [1, 5, 64, 1024])
@pytest.mark.parametrize("C", [1, 64, 300])
@pytest.mark.parametrize("dc,du", SHAPES)
def test_every_block_equals_the_oracle(device, dc, du, C, k):
    gm, X, seg, vt, cands, kinds, ora = _case(device, dc, du, C)
    top = gm.acquire_topk(cands, k)
    assert len(top) == gm.B and top.k == k and top.index.shape == (gm.B, k)
    for b in range(gm.B):
        kind = kinds.get(b)
        if kind == "no_model" or kind == "unsupported":
            assert top.count[b] == 0 and top.shortlist[b] == 0, (b, kind)
            assert top.flags[b] == (NO_MODEL if kind == "no_model" else UNSUPPORTED), (b, kind, top.flags[b])
            assert np.all(top.index[b] == -1) and np.all(np.isnan(top.score[b]))
            continue
        assert not top.flags[b] & (NO_MODEL | UNSUPPORTED), (b, kind)
        _check_block(top, b, ora[b], k, (dc, du, C, kind))
        if kind == "const_cont":
            assert top.count[b] == 0 and len(ora[b][3]) == 0
        if kind == "one_level":
            assert top.flags[b] & OVERFLOW and top.shortlist[b] == C  # exact-only: every candidate re-scored
        if kind == "all_far":
            assert top.count[b] == min(k, C) and np.all(top.score[b, :top.count[b]] == 1.0)
            np.testing.assert_array_equal(top.index[b, :top.count[b]], np.arange(min(k, C)))


@pytest.mark.parametrize("C", [1, 64, 300])
@pytest.mark.parametrize("dc,du", SHAPES)
def test_k1_is_the_grouped_pick(device, dc, du, C):
    gm, X, seg, vt, cands, kinds, ora = _case(device, dc, du, C)
    picks = gm.acquire(cands)
    top = gm.acquire_topk(cands, 1)
    for b in range(gm.B):
        assert (top.count[b] == 0) == (picks.index[b] == -1), (b, kinds.get(b))
        if top.count[b]:
            assert top.index[b, 0] == picks.index[b], (b, kinds.get(b))
            assert _same(top.score[b, 0], picks.score[b]) and _same(top.pdf_l[b, 0], picks.pdf_l[b]) and \
                _same(top.pdf_g[b, 0], picks.pdf_g[b]), (b, kinds.get(b))
    # entry 0 of a longer list is the same pick
    top5 = gm.acquire_topk(cands, 5)
    np.testing.assert_array_equal(top5.index[:, 0], picks.index)


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("dc,du", [(5, 2), (24, 8)])
def test_the_single_path_agrees(device, dc, du, k):
    C = 64
    gm, X, seg, vt, cands, kinds, ora = _case(device, dc, du, C)
    top = gm.acquire_topk(cands, k)
    for b in (3, 5, 6, 9, 10, 17):  # signed, plain, all-far, the two long ones, plain
        t1 = gm.pair(b).acquire_topk(cands[b], k)
        assert top.count[b] == t1.count, (b, top.count[b], t1.count)
        c = t1.count
        np.testing.assert_array_equal(top.index[b, :c], t1.index, err_msg=str(b))
        np.testing.assert_array_equal(top.score[b, :c].view(np.int64), t1.score.view(np.int64), err_msg=str(b))
        np.testing.assert_array_equal(top.pdf_l[b, :c], t1.pdf_l, err_msg=str(b))
        np.testing.assert_array_equal(top.pdf_g[b, :c], t1.pdf_g, err_msg=str(b))


def test_ties_at_the_cut(device):
    """One group's oracle winner copied to 7 scattered later indices: 8 bit-equal best scores.  Every cut from 1 to
    10 falls inside, at the end of or past the tie; equal scores come out smallest index first and NEAR_TIE is set
    (inside the tie by the adjacent pair or the entry left out, past it by the adjacent pairs returned)."""
    dc, du, C = 5, 2, 64
    gm, X, seg, vt, cands0, kinds, ora = _case(device, dc, du, C)
    # a plain group whose winner leaves room for 7 later copies
    b = next(b for b in range(11, gm.B) if kinds.get(b) is None and 0 <= ora[b][3][0] <= C - 9)
    w = int(ora[b][3][0])
    later = w + 1 + (np.arange(7) * (C - 1 - w)) // 7
    assert len(set(later.tolist())) == 7 and later.min() > w and later.max() < C
    cands = cands0.copy()
    cands[b, later] = cands[b, w]
    l, g = _oracle(gm, X, seg, vt, cands, b)
    s, order = _ranked(l, g)
    tied = np.sort(np.concatenate([[w], later]))
    np.testing.assert_array_equal(order[:8], tied)
    assert np.all(s[tied].view(np.int64) == s[w].view(np.int64))
    for k in range(1, 11):
        top = gm.acquire_topk(cands, k)
        _check_block(top, b, (l, g, s, order), k, "ties")
        np.testing.assert_array_equal(top.index[b, :min(k, 8)], tied[:k])
        assert top.flags[b] & NEAR_TIE, k
        for o in [o for o in (11, 12, 13) if o != b][:2]:  # the other groups are untouched by the edit
            _check_block(top, o, ora[o], k, "ties-other")


def test_the_block_of_ones(device):
    """A pool whose rows 40.. are far from every observation: their scores are exactly 1, so the top-k past the few
    scores below 1 is a run of exact ties in index order.  The all-far group states the first-k rule: where the
    one-pick call's screen certified every candidate as exactly 1 (its shortlist is 1), the top-k re-scores only the
    first min(k, C) of them."""
    dc, du, C = 8, 0, 300
    from hpbandster_amd import groups
    X, losses, seg, vt, levels, cands, kinds = _groups(dc, du, C)
    gm = groups.fit_groups(X, losses, seg, vt, device=device)
    b = 7
    assert kinds.get(b) is None
    cands[b, 40:, :] = 4.0 + np.random.RandomState(77).rand(C - 40, dc)
    l, g = _oracle(gm, X, seg, vt, cands, b)
    s, order = _ranked(l, g)
    assert np.all(s[40:] == 1.0)
    nsub = int((s < 1.0).sum())
    assert nsub < 64
    ones = np.nonzero(s == 1.0)[0]
    picks = gm.acquire(cands)
    for k in (64, 300):
        top = gm.acquire_topk(cands, k)
        _check_block(top, b, (l, g, s, order), k, "ones")
        upto = min(k, nsub + len(ones))
        assert np.all(top.score[b, nsub:upto] == 1.0)
        np.testing.assert_array_equal(top.index[b, nsub:upto], ones[:upto - nsub])
        if k == 64:
            assert top.flags[b] & NEAR_TIE
        # the all-far group, against the existing call
        la, ga = _oracle(gm, X, seg, vt, cands, 6)
        _check_block(top, 6, (la, ga) + _ranked(la, ga), k, "all_far")
        if picks.shortlist[6] == 1:
            assert top.shortlist[6] == min(k, C), (k, top.shortlist[6])
        print("ones: k %d, group %d: %d scores below 1, shortlist %d; all-far shortlist %d (one-pick %d)" % (
            k, b, nsub, top.shortlist[b], top.shortlist[6], picks.shortlist[6]))


def test_past_the_lds_array(device):
    """B = 4, C = 2500, k = 1024: the ranking's LDS array (2048 entries) fills and merges; group 2 is exact-only, so
    all its 2500 candidates pass through the running best."""
    from oracle import c_oracle
    from hpbandster_amd import groups
    dc, du, C, k, B = 5, 2, 2500, 1024, 4
    rs = np.random.RandomState(31)
    D = dc + du
    lens = np.array([60, 90, 75, 120])
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Nt = int(seg[-1])
    X = np.hstack([rs.rand(Nt, dc), rs.randint(0, 4, (Nt, du)).astype(np.float64)])
    X[seg[2]:seg[3], dc] = 1.0  # one observed level: exact-only
    vt = "c" * dc + "u" * du
    gm = groups.fit_groups(X, rs.rand(Nt), seg, vt, device=device)
    cands = np.hstack([rs.rand(B * C, dc), rs.randint(0, 4, (B * C, du)).astype(np.float64)]).reshape(B, C, D)
    cands[:, ::7, :dc] = 4.0 + rs.rand(B, len(range(0, C, 7)), dc)  # exact 1s scattered through every pool
    cands[2, :, dc] = np.where(np.arange(C) % 5 == 3, 0.0, 1.0)  # the exact-only group: a mismatch scores NaN
    cands[2, 100:1500] = cands[2, 50]  # a run of bit-equal scores longer than k in the exact-only group
    top = gm.acquire_topk(cands, k)
    for b in range(B):
        l, g = _oracle(gm, X, seg, vt, cands, b)
        _check_block(top, b, (l, g) + _ranked(l, g), k, "lds")
    np.testing.assert_array_equal(top.count, k)
    assert top.flags[2] & OVERFLOW and top.shortlist[2] == C
    assert not top.flags[0] & OVERFLOW


def test_determinism_and_no_crosstalk(device):
    import torch
    from hpbandster_amd import kde
    dc, du, C, k = 5, 2, 64, 5
    gm, X, seg, vt, cands, kinds, ora = _case(device, dc, du, C)
    step = kde.TOPK_HEAD_BYTES + kde.TOPK_REC.itemsize * k

    def blocks(c):
        raw = gm.acquire_topk(c, k, sync=False).cpu().numpy()
        assert raw.shape == (gm.B, step)
        out = []
        for b in range(gm.B):
            count = int(raw[b, :4].view("<i4")[0])
            out.append(raw[b, :kde.TOPK_HEAD_BYTES + kde.TOPK_REC.itemsize * count].tobytes())
        return out

    a, a2 = blocks(cands), blocks(cands)
    assert a == a2  # headers and the records up to count, byte for byte
    c7 = cands.copy()
    c7[7] = c7[7][::-1]
    c = blocks(c7)
    assert c[7] != a[7]
    for b in range(gm.B):
        if b != 7:
            assert c[b] == a[b], b
    torch.cuda.synchronize(device)


def test_python_surface(device):
    import torch
    from hpbandster_amd import groups, kde
    from hpbandster_amd import synthetic as S
    dc, du, D, k = 4, 2, 6, 3
    lens = np.array([40, 3, 90, 6, 64])  # groups 1 and 3: rows <= D, no model
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    X = S.make_observations(int(seg[-1]), dc, du, 3, seed=5)
    losses = S.make_losses(int(seg[-1]), seed=6)
    gm = groups.fit_groups(X, losses, seg, S.var_type_string(dc, du), device=device)
    levels = [0] * dc + [3] * du
    rows, top = gm.propose(32, seed=4, levels=levels, topk=k)
    assert isinstance(top, groups.GroupTopK) and rows.shape == (5, k, D)
    cands, _ = gm.sample(32, seed=4, levels=levels)
    ch = cands.cpu().numpy()
    for b in range(5):
        if not gm.has_model[b]:
            assert top.count[b] == 0 and top.flags[b] & NO_MODEL and np.all(np.isnan(rows[b]))
            continue
        assert top.count[b] == k
        np.testing.assert_array_equal(rows[b], ch[b, top.index[b]])
        assert isinstance(top.top(b), kde.TopK) and top.top(b).count == k
    rows1, picks = gm.propose(32, seed=4, levels=levels)
    np.testing.assert_array_equal(top.index[:, 0], picks.index)
    np.testing.assert_array_equal(rows[gm.has_model, 0], rows1[gm.has_model])
    with pytest.raises(Exception):
        gm.propose(32, seed=4, levels=levels, topk=k, requests=2)
    with pytest.raises(ValueError):
        gm.acquire_topk(cands, 0)
    with pytest.raises(ValueError):
        gm.acquire_topk(cands, 1025)
    # sync=False: the device tensor of the blocks; a side stream and a caller's workspace
    st = torch.cuda.Stream(device=device)
    ws = torch.empty(gm.workspace_bytes_topk(32, k), dtype=torch.uint8, device=device)
    assert gm.workspace_bytes_topk(32, k) >= gm.workspace_bytes(32)
    torch.cuda.synchronize(device)
    res = gm.acquire_topk(cands, k, stream=st, workspace=ws, sync=False)
    assert res.is_cuda and tuple(res.shape) == (5, 16 + 40 * k)
    st.synchronize()
    t2 = groups.GroupTopK.from_bytes(res.cpu().numpy().tobytes(), 5, k)
    np.testing.assert_array_equal(t2.index, top.index)
    np.testing.assert_array_equal(t2.score.view(np.int64), top.score.view(np.int64))
    with pytest.raises(Exception):
        gm.acquire_topk(cands, k, workspace=ws[:gm.workspace_bytes(32)])
    # C = 0: B headers with count 0 and k filled in; k > C
    raw0 = gm.acquire_topk(np.empty((5, 0, D)), k, sync=False).cpu().numpy()
    np.testing.assert_array_equal(raw0[:, :16].copy().view("<i4").reshape(5, 4), [[0, 0, 0, k]] * 5)
    t0 = gm.acquire_topk(ch[:, :2].copy(), k)
    np.testing.assert_array_equal(t0.count, np.where(gm.has_model, 2, 0))
    # B = 0
    g0 = groups.fit_groups(np.empty((0, D)), np.empty(0), np.zeros(1, np.int64), S.var_type_string(dc, du),
                           device=device)
    r0, tk0 = g0.propose(8, 1, levels, topk=k)
    assert r0.shape == (0, k, D) and len(tk0) == 0
