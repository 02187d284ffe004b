"""Grouped log-ratio ranking on the GPU: hbx_kde_rank_groups (groups.rank_values) against np.lexsort byte for byte,
hbx_kde_rank_logratio_groups (GroupModel.rank_logratio, propose(score="log_ratio")) against the fp64 log-space oracle.
"""
import functools

import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

NO_MODEL, UNSUPPORTED = 16, 32
# (C, k): one candidate, k = C, a full wave, one past it (the 8-byte loads at a range's end, odd rows off the 16-byte
# phase), a second step of the 4-wave instance, the LDS instance at k = 1024 and with several merges, and sliced pools
# (two launches) through either instance
SHAPES = [(1, 1), (5, 5), (64, 64), (65, 1), (65, 64), (65, 65), (257, 3), (1025, 1024), (4099, 130), (40000, 8),
          (40000, 70)]
KINDS = ["random", "descending", "ascending", "equal", "special", "no_model"]
B = 3


def _inputs(kind, C, k):
    """ln_l, ln_g [B, C] and status [B]; every group's values differ from its neighbours'"""
    rs = np.random.RandomState(1000 + C + k)
    ln_l = np.round(rs.randn(B, C) * 3, 1)  # (one decimal: many equal scores in a long pool)
    ln_g = np.round(rs.randn(B, C) * 3, 1)
    status = np.zeros(B, dtype=np.int32)
    ramp = np.arange(C, dtype=np.float64)[None, :] * (1.0 + np.arange(B))[:, None]
    if kind == "descending":  # every candidate beats the threshold: the staging buffer flushes as often as it can
        ln_l, ln_g = ramp, np.zeros((B, C))
    elif kind == "ascending":
        ln_l, ln_g = -ramp, np.zeros((B, C))
    elif kind == "equal":
        ln_l, ln_g = np.zeros((B, C)), np.arange(B, dtype=np.float64)[:, None] * np.ones((1, C))
    elif kind == "special":
        vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.0])
        ln_l, ln_g = vals[rs.randint(0, 7, size=(B, C))], vals[rs.randint(0, 7, size=(B, C))]
        ln_l[1], ln_g[1] = np.nan, 0.0  # fewer than k values that are not NaN: k - 1 of them
        ln_l[1, :k - 1] = rs.randn(k - 1)
        ln_l[2] = np.nan  # none
    elif kind == "no_model":
        status[:] = [0, NO_MODEL, UNSUPPORTED]
    return np.ascontiguousarray(ln_l), np.ascontiguousarray(ln_g), status


def _reference(ln_l, ln_g, status, k):
    with np.errstate(invalid="ignore"):
        s = ln_g - ln_l
    C = s.shape[1]
    index = np.full((B, k), -1, dtype=np.int32)
    out = [np.full((B, k), np.nan) for _ in range(3)]
    count = np.zeros(B, dtype=np.int32)
    for b in range(B):
        if status[b] & (NO_MODEL | UNSUPPORTED):
            continue
        nan = np.isnan(s[b])
        cls = np.where(nan, 2, np.where(s[b] == np.inf, 1, 0))
        key = np.where(nan | (s[b] == 0), 0.0, s[b])  # (-0 -> +0)
        order = np.lexsort((np.arange(C), key, cls))
        count[b] = min(k, int((~nan).sum()))
        top = order[:count[b]]
        index[b, :count[b]] = top
        for o, v in zip(out, (s[b], ln_l[b], ln_g[b])):
            o[b, :count[b]] = v[top]
    return (index, count) + tuple(out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,k", SHAPES)
def test_rank_values_against_lexsort(device, C, k, kind):
    from hpbandster_amd import groups
    ln_l, ln_g, status = _inputs(kind, C, k)
    index, count, s, l, g = _reference(ln_l, ln_g, status, k)
    r = groups.rank_values(ln_l, ln_g, k, status, device=device)
    np.testing.assert_array_equal(r.count, count)
    np.testing.assert_array_equal(r.status, status)
    np.testing.assert_array_equal(r.index, index)
    for name, want in (("score", s), ("ln_l", l), ("ln_g", g)):
        assert getattr(r, name).tobytes() == want.tobytes(), name
    raw = [groups.rank_values(ln_l, ln_g, k, status, device=device, sync=False).cpu().numpy().tobytes() for _ in range(2)]
    assert raw[0] == raw[1]
    if kind == "special":
        assert count[1] == k - 1 and count[2] == 0
    if kind == "no_model":
        assert list(r.count) == [k, 0, 0]


@functools.lru_cache(maxsize=None)
def _model(device, dc, du, lens, seed):
    """B small brackets fitted on the device: (gm, levels, oracle(cands) -> (ln l, ln g) [B, C])"""
    from hpbandster_amd import groups
    from hpbandster_amd import synthetic as S
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    X = S.make_observations(int(seg[-1]), dc, du, 3, seed=seed)
    vt = S.var_type_string(dc, du)
    gm = groups.fit_groups(X, S.make_losses(int(seg[-1]), seed=seed + 1), seg, vt, device=device)
    bws, nls = gm.bandwidths(), (gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy())

    def oracle(cands):
        return tuple(np.stack([O.log_pdf_many(X[seg[b]:seg[b + 1]][gm.rows_of(b)[kd]], bws[kd][b], vt, cands[b],
                                              nls[kd][b]) for b in range(gm.B)]) for kd in (0, 1))
    return gm, [0] * dc + [3] * du, oracle


def _check_against_oracle(r, ol, og, k, rtol=1e-5):
    """The issue's margins: t_i = rtol (max(1, |ln l_i|) + max(1, |ln g_i|)) from the oracle's values"""
    so = og - ol
    t = rtol * (np.maximum(1.0, np.abs(ol)) + np.maximum(1.0, np.abs(og)))
    for b in range(len(r)):
        assert r.count[b] == k
        top = r.index[b]
        for got, ref in ((r.ln_l[b], ol[b, top]), (r.ln_g[b], og[b, top])):
            assert np.all(np.abs(got - ref) <= rtol * np.maximum(1.0, np.abs(ref))), b
        order = np.argsort(so[b], kind="stable")
        a, c = order[k - 1], order[k]  # the seeds keep the oracle's own cut clear of the margin
        print("group %d: oracle gap %.3g, margin %.3g" % (b, so[b, c] - so[b, a], t[b, a] + t[b, c]))
        assert so[b, c] - so[b, a] > t[b, a] + t[b, c], b
        assert set(top) == set(order[:k]), (b, top, order[:k])
        rest = np.setdiff1d(np.arange(so.shape[1]), top)
        assert np.all(so[b, rest] >= so[b, top[-1]] - (t[b, rest] + t[b, top[-1]])), b
        assert np.all(so[b, top[1:]] >= so[b, top[:-1]] - (t[b, top[1:]] + t[b, top[:-1]])), b


@pytest.mark.parametrize("dc,du", [(6, 0), (4, 3)])
def test_composite_against_the_oracle(device, dc, du):
    from hpbandster_amd import synthetic as S
    C, k = 200, 8
    gm, _, oracle = _model(device, dc, du, (40, 55, 70), 51)
    cands = S.make_candidates(gm.B * C, dc, du, 3, seed=53).reshape(gm.B, C, dc + du)
    r = gm.rank_logratio(cands, k)
    lp = gm.logpdf(cands)
    assert np.all(lp.status == 0) and np.all(r.status == 0)
    for b in range(gm.B):  # the ln-pdf call's own values, byte for byte
        assert r.ln_l[b].tobytes() == lp.ln_l[b, r.index[b]].tobytes()
        assert r.ln_g[b].tobytes() == lp.ln_g[b, r.index[b]].tobytes()
        assert r.score[b].tobytes() == (lp.ln_g[b, r.index[b]] - lp.ln_l[b, r.index[b]]).tobytes()
    _check_against_oracle(r, *oracle(cands), k=k)
    np.testing.assert_array_equal(r.rows(cands)[1, 0], cands[1, r.index[1, 0]])


def test_log_ratio_ranks_where_the_floored_ratio_cannot(device):
    """D = 32 (24c + 8u): every candidate's l and g lie under the floor 1e-8, the floored score is 1 throughout and
    top-k returns the lowest indices; the log ratio returns the oracle's best."""
    C, k, seed = 64, 4, 7
    gm, levels, oracle = _model(device, 24, 8, (60, 80), 61)
    cands = gm.sample(C, seed, levels)[0].cpu().numpy()
    ol, og = oracle(cands)
    assert ol.max() < np.log(1e-8) and og.max() < np.log(1e-8)
    _, top = gm.propose(C, seed, levels, topk=k)
    assert np.all(top.index == np.arange(k)[None, :]) and np.all(top.score == 1.0)
    rows, r = gm.propose(C, seed, levels, topk=k, score="log_ratio")
    _check_against_oracle(r, ol, og, k=k)
    for b in range(gm.B):
        assert set(r.index[b]) != set(range(k)), b
        np.testing.assert_array_equal(rows[b], cands[b, r.index[b]])
