"""The two acquisition rules as parameters (include/hbx.h, hbx_rules): the score floor ``pdf_floor`` f of
max(f, g) / max(l, f) and the lower limit ``min_bandwidth`` m of every fitted bandwidth, on every surface -- the
single pair (argmin, batched, top-k, staged), the grouped calls, the fits, the drop-in generators.

Expected values never come from the engine: both pdfs from the C oracle in the reference's arithmetic
(oracle.c_oracle.kde_pdf(..., exact=True)) at bandwidths this file clips itself (np.where(bw < m, m, bw)), and a
selection written here (_scores, _argmin, _topk).  Index, score and both pdfs are compared bit for bit.

Every floor case first asserts from the oracle's pdfs that the pool has candidates below and above every floor it
uses and between each two neighbouring ones, so each floor decides something.
"""
import struct

import numpy as np
import pytest

from oracle import c_oracle
from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

FLOORS = (1e-8, 1e-32, 1e-3, 1e-100)
NEAR_TIE, OVERFLOW = 2, 1
SRC_MODEL, SRC_NO_SCORE = 0, 3


# ---- the selection, restated ----------------------------------------------------------------------------------
def _scores(l, g, f):
    """(g > f ? g : f) / (f > l ? f : l) in fp64 IEEE: a NaN g gives f, a NaN l gives NaN, an l of +inf gives 0."""
    l, g = np.asarray(l, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(g > f, g, f) / np.where(f > l, f, l)


def _argmin(s):
    """strict '<' against best = +inf in index order: the first index of the smallest score below +inf, or -1"""
    best, at = np.inf, -1
    for i, v in enumerate(s):
        if v < best:
            best, at = v, i
    return at


def _topk(s, k):
    """the first k of the candidates whose score is not NaN, ascending by (score, index)"""
    idx = np.nonzero(s == s)[0]
    return idx[np.lexsort((idx, s[idx]))][:k]


def _bits(x):
    return struct.pack("<d", float(x))


def _spans(p, floors, what):
    """The pdfs p decide something at every floor: values below the smallest, above the largest, and between each
    two neighbours."""
    p = p[p == p]
    fs = sorted(floors)
    assert (p < fs[0]).any(), (what, "nothing below", fs[0])
    assert (p > fs[-1]).any(), (what, "nothing above", fs[-1], p.max())
    for a, b in zip(fs, fs[1:]):
        assert ((p > a) & (p < b)).any(), (what, "nothing between", a, b)


def _check_pick(res, l, g, f, where):
    s = _scores(l, g, f)
    want = _argmin(s)
    assert want >= 0 and res.index == want, (where, res, want, s[want])
    assert _bits(res.score) == _bits(s[want]), (where, res, s[want])
    assert _bits(res.pdf_l) == _bits(l[want]) and _bits(res.pdf_g) == _bits(g[want]), (where, res)
    return want


def _check_topk(top, l, g, f, k, where):
    s = _scores(l, g, f)
    want = _topk(s, k)
    assert top.count == len(want), (where, top.count, len(want))
    for j, i in enumerate(want):
        assert top.index[j] == i, (where, j, top.index[:top.count], want)
        assert _bits(top.score[j]) == _bits(s[i]), (where, j)
        assert _bits(top.pdf_l[j]) == _bits(l[i]) and _bits(top.pdf_g[j]) == _bits(g[i]), (where, j)


# ---- models and pools ------------------------------------------------------------------------------------------
def _pool(rs, Xg, n, dc, du, lev, n_far):
    """A pool whose pdfs span every floor: good rows perturbed a little (the largest l), uniform points, and points
    at coordinate 3.0 in 1 .. n_far continuous dims (l down to below 1e-100), in one random order."""
    D = dc + du
    P = np.empty((n, D))
    P[:, :dc] = rs.rand(n, dc)
    for u in range(du):
        P[:, dc + u] = rs.randint(0, lev, size=n)
    k = rs.rand(n)
    near = k < 0.35
    src = Xg[rs.randint(0, len(Xg), size=n)]
    P[near] = src[near]
    P[near, :dc] += rs.choice([1e-3, 0.02, 0.1, 0.25], size=(int(near.sum()), 1)) * rs.randn(int(near.sum()), dc)
    far = k > 0.85
    for i in np.nonzero(far)[0]:
        P[i, rs.choice(dc, size=rs.randint(1, min(n_far, dc) + 1), replace=False)] = 3.0
    return np.ascontiguousarray(P)


class _Case(object):
    """One model (explicit split and bandwidths, so the pair can be rebuilt under every floor), one pool, the
    oracle's pdfs of the pool."""

    def __init__(self, dc, du, lev, n_obs, n_cand, seed, cat_bw, n_far, device, uniform=0):
        from hpbandster_amd import synthetic as S
        self.vt = S.var_type_string(dc, du)
        self.X = S.make_observations(n_obs, dc, du, lev, seed=seed) if du else \
            np.ascontiguousarray(np.random.RandomState(seed).rand(n_obs, dc))
        losses = S.make_losses(n_obs, seed=seed + 1)
        self.g_idx, self.b_idx = O.bohb_split(self.X, losses, dc + du + 1)
        cat = np.array([v == "u" for v in self.vt])
        self.bwg, self.bwb = O.normal_reference_bw(self.X[self.g_idx]), O.normal_reference_bw(self.X[self.b_idx])
        if cat_bw is not None:  # > 0: capped there (an unsigned pair); < 0: set to -cat_bw (1.2: a signed pair)
            self.bwg[cat] = np.minimum(self.bwg[cat], cat_bw) if cat_bw > 0 else -cat_bw
            self.bwb[cat] = np.minimum(self.bwb[cat], cat_bw) if cat_bw > 0 else -cat_bw
        self.nlg, self.nlb = O.num_levels(self.X[self.g_idx], self.vt), O.num_levels(self.X[self.b_idx], self.vt)
        rs = np.random.RandomState(seed + 2)
        self.C = _pool(rs, self.X[self.g_idx], n_cand, dc, du, lev, n_far)
        if uniform:  # the leading candidates: the synthetic uniform pool (the floor-dependent pick of the issue)
            self.C[:uniform] = S.make_candidates(uniform, dc, du, lev)
        with np.errstate(all="ignore"):
            self.l = c_oracle.kde_pdf(self.X[self.g_idx], self.bwg, self.vt, self.nlg, self.C, exact=True)
            self.g = c_oracle.kde_pdf(self.X[self.b_idx], self.bwb, self.vt, self.nlb, self.C, exact=True)
        self.device = device
        self._pairs = {}
        self._Cd = None

    def pair(self, f=None):
        from hpbandster_amd import kde
        if f not in self._pairs:
            kw = {} if f is None else {"pdf_floor": f}
            self._pairs[f] = kde.fit_pair_from_rows(self.X, self.g_idx, self.b_idx, self.vt, self.bwg, self.bwb,
                                                    self.nlg, self.nlb, device=self.device, **kw)
        return self._pairs[f]

    def Cd(self):
        import torch
        if self._Cd is None:
            self._Cd = torch.from_numpy(self.C).to(self.device)
        return self._Cd


_CASES = {}
# name: (dc, du, levels, observations, candidates, seed, categorical bandwidth, far dims, uniform head)
_SPECS = {
    "6c2u": (6, 2, 4, 300, 512, 11, 0.8, 6, 0),            # the coarse h32 family
    "24c8u": (24, 8, 4, 1500, 4096, 1, 0.5, 8, 256),       # config #1's shape; candidates 0..255 uniform
    "3c1u": (3, 1, 4, 1000, 515, 21, 0.8, 3, 0),           # fewer than 5 continuous dims: the f32 kernels
    "signed": (8, 4, 4, 300, 700, 31, -1.2, 8, 0),         # categorical bandwidth 1.2: negative match factors
}


def _case(name, device):
    if name not in _CASES:
        dc, du, lev, n, nc, seed, cb, nf, uni = _SPECS[name]
        _CASES[name] = _Case(dc, du, lev, n, nc, seed, cb, nf, device, uniform=uni)
    return _CASES[name]


def _usable_floors(case):
    """Every floor of FLOORS, with the assertion that the pool's good-KDE pdfs span them all."""
    _spans(case.l, FLOORS, "l")
    g = case.g[case.g == case.g]
    assert (g < min(FLOORS)).any() and (g > 1e-8).any(), (g.min(), g.max())
    return FLOORS


# ---- floors: the single surface --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_SPECS))
def test_floors_single_surface(device, name):
    """acquire, acquire_batch (seg 64) and acquire_topk (k = 8) under every floor: the oracle's picks bit for bit;
    pdf_floor=1e-8 gives the records of the calls without the keyword, byte for byte."""
    from hpbandster_amd import kde
    case = _case(name, device)
    floors = _usable_floors(case)
    base = case.pair(None)
    print(name, "variants", base.good.variant, base.bad.variant, "l range", np.nanmin(case.l), np.nanmax(case.l))
    if name == "signed":
        assert base.good.has_neg and base.bad.has_neg
    if name == "3c1u":
        assert not (base.good.variant >> 4) & 1  # not the f16 matrix-core kernels
    if name == "24c8u":
        assert (base.good.variant >> 7) & 1 and (base.bad.variant >> 7) & 1  # the coarse 32x32 instance
    Cd, nc, seg, k = case.Cd(), len(case.C), 64, 8
    picks = {}
    for f in floors:
        pair = case.pair(f)
        assert pair.pdf_floor == f
        res = pair.acquire(Cd)
        picks[f] = _check_pick(res, case.l, case.g, f, (name, f, "acquire"))
        recs = pair.acquire_batch(Cd, seg)
        assert len(recs) == (nc + seg - 1) // seg
        for b, r in enumerate(recs):
            _check_pick(r, case.l[b * seg:(b + 1) * seg], case.g[b * seg:(b + 1) * seg], f, (name, f, "batch", b))
        top = pair.acquire_topk(Cd, k)
        _check_topk(top, case.l, case.g, f, k, (name, f, "topk"))
    # the default floor named: the very records of the calls without it
    named, plain = case.pair(1e-8), base
    a, b = named.acquire(Cd), plain.acquire(Cd)
    assert struct.pack(kde.RESULT_FMT, a.index, a.score, a.rel, a.flags, a.shortlist, a.near, a.pdf_l, a.pdf_g) == \
        struct.pack(kde.RESULT_FMT, b.index, b.score, b.rel, b.flags, b.shortlist, b.near, b.pdf_l, b.pdf_g)
    ra = named.acquire_batch(Cd, seg, sync=False).cpu().numpy().tobytes()
    rb = plain.acquire_batch(Cd, seg, sync=False).cpu().numpy().tobytes()
    assert ra == rb
    ta, tb = named.acquire_topk(Cd, k), plain.acquire_topk(Cd, k)
    for fld in ("index", "score", "pdf_l", "pdf_g", "rel"):
        assert getattr(ta, fld)[:ta.count].tobytes() == getattr(tb, fld)[:tb.count].tobytes(), fld
    assert (ta.count, ta.shortlist, ta.flags) == (tb.count, tb.shortlist, tb.flags)
    if name == "24c8u":
        # the floor decides what is proposed: over the 256 uniform candidates of config #1's shape the pick under
        # the snapshot's 1e-8 is not the pick under 1e-32 (C oracle: candidates 207 and 84) -- and the engine follows
        lu, gu = case.l[:256], case.g[:256]
        w8, w32 = _argmin(_scores(lu, gu, 1e-8)), _argmin(_scores(lu, gu, 1e-32))
        assert w8 != w32, (w8, w32)
        import torch
        Cu = torch.from_numpy(np.ascontiguousarray(case.C[:256])).to(device)
        assert case.pair(1e-8).acquire(Cu).index == w8 and case.pair(1e-32).acquire(Cu).index == w32
        assert case.pair(None).acquire(Cu).index == w8


# ---- floors: the staged paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [1e-32, 1e-3])
def test_floors_staged(device, monkeypatch, f):
    """HBX_STAGED=2 against 0 under another floor: the argmin's and the top-k's records are equal, and the oracle's."""
    case = _case("24c8u", device)
    _spans(case.l, (f,), "l")
    pair, Cd, nc, k = case.pair(f), case.Cd(), len(case.C), 8
    import torch
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=device)
    wk = torch.empty(pair.topk_workspace_bytes(nc, k), dtype=torch.uint8, device=device)
    monkeypatch.setenv("HBX_STAGED", "0")
    off = pair.acquire(Cd, workspace=ws)
    assert not pair.acquire_stats(ws, nc)["staged"]
    toff = pair.acquire_topk(Cd, k, workspace=wk)
    monkeypatch.setenv("HBX_STAGED", "2")
    on = pair.acquire(Cd, workspace=ws)
    st = pair.acquire_stats(ws, nc)
    assert st["staged"], st
    ton = pair.acquire_topk(Cd, k, workspace=wk)
    assert pair.acquire_stats(wk, nc)["staged"]
    print("floor", f, "staged stats", st)
    for r in (on, off):
        _check_pick(r, case.l, case.g, f, (f, "staged argmin"))
    assert (on.index, _bits(on.score), _bits(on.pdf_l), _bits(on.pdf_g), on.flags, on.near) == \
        (off.index, _bits(off.score), _bits(off.pdf_l), _bits(off.pdf_g), off.flags, off.near)
    assert struct.pack("<f", on.rel) == struct.pack("<f", off.rel)
    for t in (ton, toff):
        _check_topk(t, case.l, case.g, f, k, (f, "staged topk"))
    assert (ton.count, ton.flags) == (toff.count, toff.flags)
    for fld in ("index", "score", "pdf_l", "pdf_g", "rel"):
        assert getattr(ton, fld)[:ton.count].tobytes() == getattr(toff, fld)[:toff.count].tobytes(), fld


# ---- floors: the grouped surface -----------------------------------------------------------------------------
def _ragged(dc, du, device, **kw):
    """B = 6 ragged groups, group 2 too short for a model; pools per group with pdfs on both sides of the floor."""
    from hpbandster_amd import groups
    rs = np.random.RandomState(500 + dc)
    D, lev = dc + du, 4
    lens = np.array([3 * D + 20, 2 * D + 9, D, 4 * D + 3, 2 * D + 12, 300])
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(seg[-1])
    X = np.empty((n, D))
    X[:, :dc] = rs.rand(n, dc)
    for u in range(du):
        X[:, dc + u] = rs.randint(0, lev, size=n)
    vt = "c" * dc + "u" * du
    gm = groups.fit_groups(X, rs.rand(n), seg, vt, device=device, **kw)
    np.testing.assert_array_equal(gm.has_model, [True, True, False, True, True, True])
    return gm, X, seg, vt, [0] * dc + [lev] * du


def _group_oracle(gm, X, seg, vt, b, pts):
    bwg, bwb = gm.bandwidths()
    nlg, nlb = gm.nlev_good.cpu().numpy(), gm.nlev_bad.cpu().numpy()
    g_rows, b_rows = gm.rows_of(b)
    Xb = X[seg[b]:seg[b + 1]]
    with np.errstate(all="ignore"):
        return (c_oracle.kde_pdf(Xb[g_rows], bwg[b], vt, nlg[b], pts, exact=True),
                c_oracle.kde_pdf(Xb[b_rows], bwb[b], vt, nlb[b], pts, exact=True))


@pytest.mark.parametrize("dc,du", [(6, 2), (24, 8)])
def test_floors_grouped_surface(device, dc, du):
    """acquire (C = 64), acquire_requests (S = 3) and acquire_topk (k = 4) of a model fitted with pdf_floor=1e-32:
    every record the oracle's under that floor; get_config is sample -> acquire_requests -> finish, byte for byte."""
    from hpbandster_amd import groups
    f, C, S, k = 1e-32, 64, 3, 4
    gm, X, seg, vt, levels = _ragged(dc, du, device, pdf_floor=f)
    assert gm.pdf_floor == f and gm.min_bandwidth == 0.0
    B, D = gm.B, dc + du
    rs = np.random.RandomState(77)
    cands = np.empty((B, S, C, D))
    for b in range(B):
        Xb = X[seg[b]:seg[b + 1]]
        src = Xb[gm.rows_of(b)[0]] if gm.has_model[b] else Xb
        cands[b] = _pool(rs, src, S * C, dc, du, 4, min(dc, 8)).reshape(S, C, D)
    pdfs = {b: _group_oracle(gm, X, seg, vt, b, cands[b].reshape(S * C, D)) for b in range(B) if gm.has_model[b]}
    lall = np.concatenate([pdfs[b][0] for b in pdfs])
    _spans(lall, (1e-32, 1e-8), "grouped l")
    differs = 0
    one = gm.acquire(cands[:, 0])
    req = gm.acquire_requests(cands)
    top = gm.acquire_topk(np.ascontiguousarray(cands[:, 1]), k)
    for b in range(B):
        if not gm.has_model[b]:
            assert one.index[b] == -1 and one.flags[b] & 16 and np.all(req.index[b] == -1) and top.count[b] == 0
            continue
        l, g = (p.reshape(S, C) for p in pdfs[b])
        for s in range(S):
            sc = _scores(l[s], g[s], f)
            want = _argmin(sc)
            differs += want != _argmin(_scores(l[s], g[s], 1e-8))
            for rec, at in ((req, (b, s)),) + (((one, b),) if s == 0 else ()):
                assert rec.index[at] == want, (b, s, rec.index[at], want)
                assert _bits(rec.score[at]) == _bits(sc[want])
                assert _bits(rec.pdf_l[at]) == _bits(l[s][want]) and _bits(rec.pdf_g[at]) == _bits(g[s][want])
        sc = _scores(l[1], g[1], f)
        want = _topk(sc, k)
        assert top.count[b] == len(want)
        for j, i in enumerate(want):
            assert top.index[b, j] == i and _bits(top.score[b, j]) == _bits(sc[i]), (b, j)
            assert _bits(top.pdf_l[b, j]) == _bits(l[1][i]) and _bits(top.pdf_g[b, j]) == _bits(g[1][i])
    assert differs > 0  # the floor decided at least one of these picks
    # get_config under the floor: the composition with the same floor, byte for byte
    seed, cb, rf = 11, 5000, 1.0 / 3
    fused = gm.get_config(C, seed, levels, requests=S, random_fraction=rf, counter_base=cb, keep_pools=True)
    sc_, err = gm.sample(C, seed, levels, counter_base=cb, requests=S)
    rec = gm.acquire_requests(sc_, sync=False)
    comp = gm.finish(sc_, rec, err, levels, rf, seed, cb)
    assert fused.cands.tobytes() == sc_.cpu().numpy().tobytes()
    picks = groups.GroupPicks.from_bytes(rec.cpu().numpy().tobytes(), B, S)
    for name in groups.GroupPicks.__slots__:
        assert getattr(fused.picks, name).tobytes() == getattr(picks, name).tobytes(), name
    assert fused.rows.tobytes() == comp.rows.tobytes() and fused.source.tobytes() == comp.source.tobytes()
    ch = sc_.cpu().numpy()
    for b in range(B):  # ... and its records are the oracle's under the floor, not under 1e-8
        if gm.has_model[b]:
            l, g = _group_oracle(gm, X, seg, vt, b, ch[b, 0])
            want = _argmin(_scores(l, g, f))
            assert picks.index[b, 0] == want and _bits(picks.score[b, 0]) == _bits(_scores(l, g, f)[want])
    # the pair built from the model carries its floor
    assert gm.pair(0).pdf_floor == f


# ---- minimum bandwidth ---------------------------------------------------------------------------------------
M = 1e-3


def _clip(bw, m):
    return np.where(bw < m, m, bw)


def _min_bw_data(rs, n, good):
    """D = 5: [0] uniform, [1] a constant continuous column, [2] a continuous column of spread 1e-5, [3] uniform,
    [4] a categorical column (4 levels) that shows ONE level in the rows ``good`` (the best losses)."""
    X = np.empty((n, 5))
    X[:, 0] = rs.rand(n)
    X[:, 1] = 0.25
    X[:, 2] = 0.5 + 1e-5 * rs.rand(n)
    X[:, 3] = rs.rand(n)
    X[:, 4] = rs.randint(0, 4, size=n)
    X[good, 4] = 2.0
    return X


def _min_bw_pool(rs, Xg, n):
    """Candidates near the good rows; the categorical column matches the single level except for some: their l is
    +inf (mismatch factor h / 0) and their score 0."""
    P = Xg[rs.randint(0, len(Xg), size=n)].copy()
    P[:, 0] += 0.05 * rs.randn(n)
    P[:, 3] += 0.05 * rs.randn(n)
    P[:, 1] += 2e-4 * rs.randn(n)
    P[:, 2] += 2e-4 * rs.randn(n)
    mis = rs.rand(n) < 0.15
    mis[:5] = False
    P[mis, 4] = rs.choice([0.0, 1.0, 3.0], size=int(mis.sum()))
    return np.ascontiguousarray(P), mis


def _pair_oracle(pair, vt, C, bwg, bwb):
    with np.errstate(all="ignore"):
        return (c_oracle.kde_pdf(pair.good.data, bwg, vt, pair.good.nlev, C, exact=True),
                c_oracle.kde_pdf(pair.bad.data, bwb, vt, pair.bad.nlev, C, exact=True))


def test_min_bandwidth_refit(device):
    """ObservationStore.refit with incremental appends (D = 5 > 1 and both sets within one tile: the fit kernel of
    the fused refit, kde_fit_col_kernel) and fit_pair over D = 1 (kde_fit_stats_kernel): bandwidths bit-equal to
    the clipped normal-reference ones, picks the oracle's -- including candidates that mismatch the good set's
    single categorical level (l = +inf, score 0: the first of them wins).  Without min_bandwidth the same data
    gives no score; m = 0 and None are the default, byte for byte."""
    from hpbandster_amd import kde
    vt, n = "ccccu", 120
    rs = np.random.RandomState(5)
    losses = rs.rand(n)
    good = np.argsort(losses)[:(15 * n) // 100]
    X = _min_bw_data(rs, n, good)
    stores = {key: kde.ObservationStore(5, vt, device=device) for key in ("m", "none", "zero", "default")}
    kws = {"m": {"min_bandwidth": M}, "none": {"min_bandwidth": None}, "zero": {"min_bandwidth": 0.0}, "default": {}}
    pairs = {}
    for lo, hi in ((0, 60), (60, 61), (61, 120)):  # appended in three steps, one of a single row
        for key, st in stores.items():
            st.add(X[lo:hi], losses[lo:hi])
            pairs[key] = st.refit(6, **kws[key])
    pm, pd = pairs["m"], pairs["default"]
    g_idx, b_idx = O.bohb_split(X, losses, 6)
    assert np.array_equal(pm.good.data, X[g_idx]) and np.array_equal(pm.bad.data, X[b_idx])
    with np.errstate(all="ignore"):
        rawg, rawb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    assert rawg[1] == 0.0 and rawg[4] == 0.0 and 0 < rawg[2] < M and rawg[0] > M  # all three kinds of column
    assert pm.good.nlev[4] == 1 and pm.bad.nlev[4] == 4
    bwg, bwb = _clip(rawg, M), _clip(rawb, M)
    assert np.asarray(pm.good.bw).tobytes() == bwg.tobytes() and np.asarray(pm.bad.bw).tobytes() == bwb.tobytes()
    assert pm.good.exact_only and not pm.bad.exact_only  # the single-level dim with h = m: decided in fp64
    for key in ("none", "zero"):  # no clip: the default's bandwidths
        assert np.asarray(pairs[key].good.bw).tobytes() == np.asarray(pd.good.bw).tobytes() == rawg.tobytes()
        assert np.asarray(pairs[key].bad.bw).tobytes() == np.asarray(pd.bad.bw).tobytes() == rawb.tobytes()
    C, mis = _min_bw_pool(np.random.RandomState(6), X[g_idx], 64)
    l, g = _pair_oracle(pm, vt, C, bwg, bwb)
    assert np.isinf(l[mis]).all() and mis.sum() >= 3 and np.isfinite(l[~mis]).all()
    s = _scores(l, g, 1e-8)
    want = _argmin(s)
    assert s[want] == 0.0 and want == np.nonzero(mis)[0][0]  # the first mismatching candidate: score g / inf = 0
    res = pm.acquire(C)
    _check_pick(res, l, g, 1e-8, "min_bandwidth acquire")
    for b, r in enumerate(pm.acquire_batch(C, 16)):
        _check_pick(r, l[16 * b:16 * b + 16], g[16 * b:16 * b + 16], 1e-8, ("min_bandwidth batch", b))
    _check_topk(pm.acquire_topk(C, 8), l, g, 1e-8, 8, "min_bandwidth topk")
    keep = ~mis  # ... and a pool without them: finite pdfs, an ordinary pick
    _check_pick(pm.acquire(np.ascontiguousarray(C[keep])), l[keep], g[keep], 1e-8, "min_bandwidth matching pool")
    # without the rule: the constant column's bandwidth is 0, every pdf NaN, no score
    r0 = pd.acquire(C)
    assert r0.index == -1 and r0.score != r0.score
    for key in ("none", "zero"):
        rk = pairs[key].acquire(C)
        assert (rk.index, rk.flags, rk.shortlist, rk.near) == (r0.index, r0.flags, r0.shortlist, r0.near)
    # D = 1: the thread-per-column fit kernel
    x1 = np.full((40, 1), 0.75)
    l1 = np.random.RandomState(8).rand(40)
    p1 = kde.fit_pair(x1, l1, "c", 2, device=device, min_bandwidth=M)
    assert np.asarray(p1.good.bw).tobytes() == np.array([M]).tobytes() == np.asarray(p1.bad.bw).tobytes()
    c1 = 0.75 + 1e-3 * np.random.RandomState(9).randn(32, 1)
    la, ga = _pair_oracle(p1, "c", c1, np.array([M]), np.array([M]))
    _check_pick(p1.acquire(c1), la, ga, 1e-8, "D = 1")
    assert kde.fit_pair(x1, l1, "c", 2, device=device).acquire(c1).index == -1


def test_min_bandwidth_fit_groups(device):
    """fit_groups: B = 6 groups of D = 5 (2 B D = 60 columns: kde_fit_col_kernel) and B = 1700 (2 B D = 17000 >=
    16384 columns: kde_fit_wave_kernel): bandwidths bit-equal to the clipped ones; picks the oracle's where the good
    set agrees on one level; without the rule no score."""
    from hpbandster_amd import groups
    vt, D, n = "ccccu", 5, 40
    for B in (6, 1700):
        rs = np.random.RandomState(B)
        losses = rs.rand(B, n)
        X = np.empty((B, n, D))
        for b in range(B):
            X[b] = _min_bw_data(rs, n, np.argsort(losses[b])[:6])
        seg = np.arange(B + 1, dtype=np.int64) * n
        gm = groups.fit_groups(X.reshape(-1, D), losses.reshape(-1), seg, vt, device=device, min_bandwidth=M)
        g0 = groups.fit_groups(X.reshape(-1, D), losses.reshape(-1), seg, vt, device=device)
        gz = groups.fit_groups(X.reshape(-1, D), losses.reshape(-1), seg, vt, device=device, min_bandwidth=0.0)
        assert gm.min_bandwidth == M and g0.min_bandwidth == 0.0
        (bg, bb), (rg, rb), (zg, zb) = gm.bandwidths(), g0.bandwidths(), gz.bandwidths()
        assert zg.tobytes() == rg.tobytes() and zb.tobytes() == rb.tobytes()
        assert bg.tobytes() == _clip(rg, M).tobytes() and bb.tobytes() == _clip(rb, M).tobytes()
        for b in (0, B // 2, B - 1):  # the unclipped ones are the reference's
            gr, br = gm.rows_of(b)
            with np.errstate(all="ignore"):
                assert rg[b].tobytes() == O.normal_reference_bw(X[b][gr]).tobytes()
                assert rb[b].tobytes() == O.normal_reference_bw(X[b][br]).tobytes()
        assert np.all(bg[:, 1] == M) and np.all(bg[:, 4] == M) and np.all(bg[:, 2] == M) and np.all(bg[:, 0] > M)
        assert np.all(gm.nlev_good.cpu().numpy()[:, 4] == 1)
        if B > 6:
            continue
        C = 64
        cands, miss = np.empty((B, C, D)), []
        for b in range(B):
            cands[b], mis = _min_bw_pool(np.random.RandomState(40 + b), X[b][gm.rows_of(b)[0]], C)
            if b % 2:  # every second group: a pool that matches the level everywhere
                cands[b, :, 4] = 2.0
                mis[:] = False
            miss.append(mis)
        picks, none = gm.acquire(cands), g0.acquire(cands)
        top = gm.acquire_topk(cands, 4)
        assert np.all(none.index == -1)  # no score without the rule (the constant column)
        for b in range(B):
            l, g = _group_oracle(gm, X.reshape(-1, D), seg, vt, b, cands[b])
            assert np.isinf(l[miss[b]]).all() and np.isfinite(l[~miss[b]]).all()
            s = _scores(l, g, 1e-8)
            want = _argmin(s)
            assert want >= 0 and picks.index[b] == want and _bits(picks.score[b]) == _bits(s[want]), (b, want)
            assert _bits(picks.pdf_l[b]) == _bits(l[want]) and _bits(picks.pdf_g[b]) == _bits(g[want])
            if miss[b].any():
                assert s[want] == 0.0 and want == np.nonzero(miss[b])[0][0]
            wk = _topk(s, 4)
            assert top.count[b] == len(wk) and list(top.index[b, :len(wk)]) == list(wk)
            assert top.score[b, :len(wk)].tobytes() == s[wk].tobytes()
            # the single path on the same model: the same record
            r1 = gm.pair(b).acquire(cands[b])
            assert r1.index == want and _bits(r1.score) == _bits(s[want])


# ---- the drop-in generators --------------------------------------------------------------------------------------
class _Job(object):
    pass


def _feed(cg, space, n, rs):
    """n results whose configurations all hold x0 at one value (a converged hyperparameter) and whose good ones
    agree on the categorical choice."""
    for k in range(n):
        cfg = space.sample_configuration().get_dictionary()
        cfg["x0"] = 0.5
        loss = float(rs.rand()) + (0.0 if cfg["c"] == "a" else 10.0)
        j = _Job()
        j.id, j.exception, j.timestamps = (0, 0, k), None, {}
        j.kwargs = {"config": cfg, "budget": 1.0}
        j.result = {"loss": loss, "info": None}
        cg.new_result(j)


@pytest.mark.parametrize("sampler", ["host", "gpu"])
def test_bohb_drop_in(device, sampler):
    """BOHB(min_bandwidth=1e-3, pdf_floor=1e-32) on a space one hyperparameter of which every observation holds
    constant: get_config is model-based and returns the oracle's selection over the candidates the call drew; with
    the default rules the same history has no score (a random configuration)."""
    from hpbandster_amd import configspace as CS
    from hpbandster_amd.config_generators import BOHB

    def make(**kw):
        space = CS.ConfigurationSpace(seed=3)
        for i in range(3):
            space.add_hyperparameter(CS.UniformFloatHyperparameter("x%d" % i, lower=-2, upper=3))
        space.add_hyperparameter(CS.CategoricalHyperparameter("c", ["a", "b", "c", "d"]))
        cg = BOHB(space, device=device, random_fraction=0.0, num_samples=64, sampler=sampler, sampler_seed=17, **kw)
        _feed(cg, space, 60, np.random.RandomState(3))
        return cg, space

    cg, space = make(min_bandwidth=1e-3, pdf_floor=1e-32)
    assert len(cg.kde_models) == 1
    pair = cg.kde_models[1.0]
    assert pair.pdf_floor == 1e-32
    vt = cg.kde_vartypes
    with np.errstate(all="ignore"):
        rawg, rawb = O.normal_reference_bw(pair.good.data), O.normal_reference_bw(pair.bad.data)
    ix = list(space.get_hyperparameter_names()).index("x0")
    assert rawg[ix] == 0.0 and rawb[ix] == 0.0
    bwg, bwb = _clip(rawg, 1e-3), _clip(rawb, 1e-3)
    assert np.asarray(pair.good.bw).tobytes() == bwg.tobytes() and np.asarray(pair.bad.bw).tobytes() == bwb.tobytes()
    np.random.seed(7)
    counter = cg._sample_counter
    cfg, info = cg.get_config(1.0)
    assert info["model_based_pick"]
    if sampler == "host":  # the call's candidates again, from the same global RNG state
        np.random.seed(7)
        np.random.rand()  # (the random-fraction draw)
        cands = np.array(cg.sample_candidates(pair["good"], cg.num_samples))
    else:  # ... from the same Philox counter
        cands = pair.good.sample(cg.vartypes, cg.bw_factor, cg.num_samples, cg.sampler_seed, counter)[0].cpu().numpy()
    l, g = _pair_oracle(pair, vt, cands, bwg, bwb)
    want = _argmin(_scores(l, g, 1e-32))
    assert want >= 0
    from hpbandster_amd.configspace import Configuration
    assert cfg == Configuration(space, vector=cands[want]).get_dictionary()
    # the snapshot's rules on the same history: the constant column's bandwidth is 0 -- no score, a random pick
    cg0, _ = make()
    assert cg0.kde_models[1.0].good.bw[ix] == 0.0
    np.random.seed(7)
    assert not cg0.get_config(1.0)[1]["model_based_pick"]


def test_group_bohb_drop_in(device):
    """GroupBOHB with the same keywords: one new_results / get_configs step is model-based (HBX_CFG_MODEL) where the
    default rules give HBX_CFG_NO_SCORE."""
    from hpbandster_amd import groups
    B, m, D = 3, 12, 4
    rs = np.random.RandomState(12)
    X = rs.rand(B, m, D)
    X[:, :, 1] = 0.5  # a converged hyperparameter
    X[:, :, 3] = rs.randint(0, 4, size=(B, m))
    losses = rs.rand(B, m)
    out = {}
    for key, kw in (("rules", dict(min_bandwidth=1e-3, pdf_floor=1e-32)), ("default", {})):
        opt = groups.GroupBOHB(B, "cccu", [0, 0, 0, 4], num_samples=32, random_fraction=0.0, seed=5, device=device,
                               **kw)
        assert opt.new_results(9.0, X, losses)
        out[key] = (opt, opt.get_configs(9.0, S=2))
    opt, cfg = out["rules"]
    gm = opt.kde_models[9.0]
    assert gm.pdf_floor == 1e-32 and gm.min_bandwidth == 1e-3
    assert np.all(gm.bandwidths()[0][:, 1] == 1e-3)
    assert np.all(cfg.source == SRC_MODEL), cfg.source
    assert np.all(out["default"][1].source == SRC_NO_SCORE), out["default"][1].source
    assert np.all(out["default"][0].kde_models[9.0].bandwidths()[0][:, 1] == 0.0)
