"""The staged single acquisition (hbx_staged.hip): the good KDE scored for every candidate, the bad KDE only for
the candidates l alone does not rule out (score >= 1e-8 / max(l, 1e-8) whatever g is).

Every case runs the same pair, candidates and workspace with HBX_STAGED=2 (staged wherever supported) and
HBX_STAGED=0 (never): index, score, pdf_l, pdf_g, flags, near and rel must be equal, `shortlist` equal or lower
by one (the first certain 1e-8/1e-8 tie, when it was pruned), and the pick the C oracle's.  hbx_kde_acquire_stats
(KDEPair.acquire_stats) proves which branch a case reached.

Categorical bandwidths are capped below 1 here: the normal-reference rule gives a few hundred observations of
4-level codes a bandwidth above 1, a signed KDE, which does not stage (its own case below).
"""
import struct

import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

CAP = 4096  # STAGED_LIST_CAP: seeds at most


def _fit(X, losses, vt, device, cat_bw=0.8, bw_good=None, bw_bad=None):
    """A pair from BOHB's split with normal-reference bandwidths, categorical ones capped at cat_bw (None: as
    the rule gives them)."""
    from hpbandster_amd import kde
    g_idx, b_idx = O.bohb_split(X, losses, X.shape[1] + 1)
    cat = np.array([v == "u" for v in vt])
    with np.errstate(all="ignore"):
        bwg, bwb = O.normal_reference_bw(X[g_idx]), O.normal_reference_bw(X[b_idx])
    if cat_bw is not None:
        bwg[cat] = np.minimum(bwg[cat], cat_bw)
        bwb[cat] = np.minimum(bwb[cat], cat_bw)
    if bw_good is not None:
        bwg = bw_good(bwg)
    if bw_bad is not None:
        bwb = bw_bad(bwb)
    nlg, nlb = O.num_levels(X[g_idx], vt), O.num_levels(X[b_idx], vt)
    return kde.fit_pair_from_rows(X, g_idx, b_idx, vt, bwg, bwb, nlg, nlb, device=device)


def _bits(x):
    return struct.pack("<d", float(x))  # NaN-safe equality of fp64 fields


def _same(on, off):
    assert on.index == off.index, (on, off)
    for f in ("score", "pdf_l", "pdf_g"):
        assert _bits(getattr(on, f)) == _bits(getattr(off, f)), (f, on, off)
    assert (on.flags, on.near) == (off.flags, off.near), (on, off)
    assert struct.pack("<f", on.rel) == struct.pack("<f", off.rel), (on, off)
    assert on.shortlist in (off.shortlist, off.shortlist - 1), (on.shortlist, off.shortlist)


def _both(pair, C, monkeypatch, device, expect_staged=True, **kw):
    """(staged record, its stats, unstaged record) of one candidate set on one workspace."""
    import torch
    Cd = torch.from_numpy(np.ascontiguousarray(C)).to(device)
    nc = len(C)
    ws = torch.empty(pair.workspace_bytes(nc), dtype=torch.uint8, device=device)
    monkeypatch.setenv("HBX_STAGED", "0")
    off = pair.acquire(Cd, workspace=ws, **kw)
    st0 = pair.acquire_stats(ws, nc)
    assert not st0["staged"] and st0["evaluated"] == nc
    monkeypatch.setenv("HBX_STAGED", "2")
    on = pair.acquire(Cd, workspace=ws, **kw)
    st = pair.acquire_stats(ws, nc)
    assert st["staged"] == expect_staged, st
    again = pair.acquire(Cd, workspace=ws, **kw)  # the same workspace again: the state starts afresh
    assert pair.acquire_stats(ws, nc) == st or st["seeds"] == CAP  # (an overflowing seed list's split may vary)
    _same(again, on)
    _same(on, off)
    return on, st, off


def _oracle_pick(pair, vt, C):
    from oracle import c_oracle
    with np.errstate(all="ignore"):
        l = c_oracle.kde_pdf(pair.good.data, pair.good.bw, vt, pair.good.nlev, C, exact=True)
        g = c_oracle.kde_pdf(pair.bad.data, pair.bad.bw, vt, pair.bad.nlev, C, exact=True)
    return O.select(l, g)[0], l, g


@pytest.fixture(scope="module")
def bench_like(device):
    """24c + 8u with 4 levels, 400 observations, 4099 candidates (no multiple of 32, 64 or 512), with the
    oracle's pdfs."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=211)
    pair = _fit(X, S.make_losses(400, seed=212), vt, device)
    C = S.make_candidates(4099, 24, 8, 4, seed=213)
    want, l, g = _oracle_pick(pair, vt, C)
    return pair, vt, C, want, l, g


def test_clamp_prunes_nearly_all(device, monkeypatch, bench_like):
    """pdfs around 1e-8 at D = 32: the candidates l rules out are nearly all.  In fp64, 8 of the 4099 candidates
    lie in the seed band l >= l_max / 4 or have an l-only bound 1e-8 / max(l, 1e-8) at or below the best score
    (0.0034); 73 % have l < 1e-8, an l-only bound of 1.  The coarse instance's wider intervals add to the 8, but
    the survivor list stays near-empty (under 2 % of the candidates) and g is evaluated for fewer than a tenth."""
    pair, vt, C, want, l, g = bench_like
    on, st, off = _both(pair, C, monkeypatch, device)
    assert on.index == want
    best = (np.maximum(g, 1e-8) / np.maximum(l, 1e-8)).min()
    need = int(((l >= l.max() / 4) | (1e-8 / np.maximum(l, 1e-8) <= best)).sum())
    print("staged stats", st, "fp64 need", need)
    assert st["evaluated"] >= need  # nothing that can win is left out
    assert st["survivors"] <= len(C) // 50, (st, need)
    assert st["evaluated"] < len(C) // 10, (st, need)
    assert 1 <= st["seeds"] < CAP


def test_nothing_pruned(device, monkeypatch):
    """8 continuous dims: every pdf far above 1e-8, so every l-only bound (a score of 1e-8 / l, far below 1)
    lies below any real score -- every candidate survives: seeds + survivors == Nc (no NaN rows)."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(8, 0)
    X = S.make_observations(300, 8, 0, 1, seed=221)
    pair = _fit(X, S.make_losses(300, seed=222), vt, device)
    C = S.make_candidates(1537, 8, 0, 1, seed=223)
    on, st, off = _both(pair, C, monkeypatch, device)
    want, l, g = _oracle_pick(pair, vt, C)
    assert l.min() > 1e-6  # the premise
    assert on.index == want
    assert st["seeds"] + st["survivors"] == len(C) and st["evaluated"] == len(C)


def test_every_score_exactly_one(device, monkeypatch):
    """Candidates far outside the observations' box in 32 dims: both pdfs below 1e-8, every score exactly
    1e-8 / 1e-8.  U_seed = ln 1 = 0 and every l-only bound is 0 too: all survive, the first index wins."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=231)
    pair = _fit(X, S.make_losses(400, seed=232), vt, device)
    C = S.make_candidates(700, 24, 8, 4, seed=233)
    C[:, :24] += 4.0
    on, st, off = _both(pair, C, monkeypatch, device)
    assert (on.index, on.score) == (0, 1.0)
    assert st["seeds"] + st["survivors"] == len(C)
    assert on.index == _oracle_pick(pair, vt, C)[0]


def test_tie_across_the_prune_line(device, monkeypatch, bench_like):
    """The best candidate's row copied to a lower and to a higher index among 1200 others: three exact ties,
    the first index wins."""
    pair, vt, C, want, l, g = bench_like
    C = C[:1200].copy()
    best = O.select(l[:1200], g[:1200])[0]
    assert best >= 0
    lo, hi = 3, 1150
    assert lo != best != hi
    C[lo] = C[best]
    C[hi] = C[best]
    on, st, off = _both(pair, C, monkeypatch, device)
    assert on.index == min(lo, best) == _oracle_pick(pair, vt, C)[0]
    assert on.near >= 3


def test_tie_overflowing_the_seed_cap(device, monkeypatch, bench_like):
    """5000 copies of the best row behind 1000 other candidates: all within a factor 4 of the best l, so the
    4096-entry seed list overflows and the rest must arrive through the survivor list -- every copy's g is
    evaluated, and the first copy (the original's index) wins."""
    pair, vt, C, want, l, g = bench_like
    base = C[:1000]
    best = O.select(l[:1000], g[:1000])[0]
    assert best >= 0
    C2 = np.vstack([base, np.repeat(base[best:best + 1], 5000, axis=0)])
    on, st, off = _both(pair, C2, monkeypatch, device)
    assert on.index == best
    assert st["seeds"] == CAP and st["survivors"] >= 5001 - CAP, st
    assert on.near >= 5001


def test_nan_l_single_level_dim(device, monkeypatch):
    """The good KDE's first categorical dim holds one observed level (its h / (c - 1) is 0 / 0 off the level):
    l is NaN for every candidate without that level -- never seeded, never a survivor, never picked."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=241)
    losses = S.make_losses(400, seed=242)
    g_idx, _ = O.bohb_split(X, losses, 33)
    X[g_idx, 24] = 2.0
    pair = _fit(X, losses, vt, device)
    assert pair.good.nlev[24] == 1
    C = S.make_candidates(2050, 24, 8, 4, seed=243)
    on, st, off = _both(pair, C, monkeypatch, device)
    want, l, g = _oracle_pick(pair, vt, C)
    nan = np.isnan(l)
    assert nan.sum() > 1000 and (~nan).sum() > 300
    assert on.index == want and not nan[on.index]
    assert st["seeds"] + st["survivors"] <= int((~nan).sum())


def test_nan_l_everywhere(device, monkeypatch):
    """A constant continuous column in the good rows (bandwidth 0, `nan_all`): l is NaN everywhere, no finite
    score, index -1 from both paths.  The pair stages: a zero bandwidth only sets the dim's scale to 0 (its
    table column is 0, |C_j| stays in range), so the good KDE keeps the coarse 32x32 table and its scoring
    kernel writes NaN estimates -- nothing is seeded, nothing survives, no g is evaluated."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=251)
    losses = S.make_losses(400, seed=252)
    g_idx, _ = O.bohb_split(X, losses, 33)
    X[g_idx, 5] = 0.25
    pair = _fit(X, losses, vt, device)
    assert pair.good.bw[5] == 0
    C = S.make_candidates(1500, 24, 8, 4, seed=253)
    assert (pair.good.variant >> 7) & 1 and (pair.bad.variant >> 7) & 1  # both on the coarse 32x32 instance
    on, st, off = _both(pair, C, monkeypatch, device)  # (asserts that HBX_STAGED=2 staged)
    assert on.index == -1 == _oracle_pick(pair, vt, C)[0]
    assert (st["seeds"], st["survivors"], st["evaluated"]) == (0, 0, 0), st


def test_rescue_markers_among_the_seeds(device, monkeypatch):
    """The bad KDE narrow in dim 0 (bandwidth 0.004) and every candidate at x_0 = 1.6, outside the observations'
    [0, 1): the rescue tests' construction, for every candidate.  Against the bad KDE x'_0 = 0.849 / 0.004 * 1.1 =
    234, so c_i <= -54000, while the probe's maximum over chunk 0 is about -X'^2 + 2 x' X' = 38000 at X' = 106: the
    shifted c_i, about -38000, is beyond the three f16 pieces' 30000 (H32_CMAX).  So every g estimate the staged
    path computes -- the seeds' first -- is a rescue marker (|C_j| <= 106^2 keeps the KDE on the 32x32 kernel),
    while l (bandwidths as fitted) ranks the candidates as usual.  A marked seed does not lower U_seed, so with
    every seed marked U_seed stays +inf and every unseeded candidate survives (l is NaN for none):
    seeds + survivors == Nc proves the merge kernel's marker branch ran, and the records' equality that the
    combine kernel rescued what it left."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=261)

    def narrow(bw):
        bw = bw.copy()
        bw[0] = 0.004
        return bw
    pair = _fit(X, S.make_losses(400, seed=262), vt, device, bw_bad=narrow)
    C = S.make_candidates(1300, 24, 8, 4, seed=263)
    C[:, 0] = 1.6
    on, st, off = _both(pair, C, monkeypatch, device)
    assert on.index == _oracle_pick(pair, vt, C)[0]
    assert st["seeds"] >= 1
    assert st["seeds"] + st["survivors"] == len(C), st


def test_index_base_and_async_fetch(device, monkeypatch, bench_like):
    """index_base = 3 * 2^33 is added to the staged pick; sync=False leaves the record on the device
    (fetch_bytes), equal to the synchronous call's."""
    import torch
    from hpbandster_amd import kde
    pair, vt, C, want, l, g = bench_like
    base = 3 * 2 ** 33
    on, st, off = _both(pair, C, monkeypatch, device, index_base=base)
    assert on.index == want + base
    Cd = torch.from_numpy(C).to(device)
    ws = torch.empty(pair.workspace_bytes(len(C)), dtype=torch.uint8, device=device)
    rv = pair.acquire(Cd, index_base=base, workspace=ws, sync=False)  # HBX_STAGED=2 still set
    rec = kde.AcqResult.from_bytes(kde.fetch_bytes(rv))
    assert pair.acquire_stats(ws, len(C))["staged"]
    _same(rec, on)
    assert rec.shortlist == on.shortlist


def test_unsupported_pairs_fall_back(device, monkeypatch):
    """HBX_STAGED=2 on pairs the staged path does not serve runs the fused path and the stats say so: a signed
    good KDE (categorical bandwidth above 1, as the normal-reference rule gives a few hundred observations) and a
    pair outside the 32x32 buckets (3 continuous dims)."""
    from hpbandster_amd import synthetic as S
    vt = S.var_type_string(24, 8)
    X = S.make_observations(400, 24, 8, 4, seed=271)
    pair = _fit(X, S.make_losses(400, seed=272), vt, device, cat_bw=None,
                bw_good=lambda bw: np.concatenate([bw[:24], np.full(8, 1.2)]))
    assert pair.good.has_neg
    C = S.make_candidates(900, 24, 8, 4, seed=273)
    on, st, off = _both(pair, C, monkeypatch, device, expect_staged=False)
    assert on.shortlist == off.shortlist and st["evaluated"] == len(C)
    vt3 = S.var_type_string(3, 0)
    X3 = S.make_observations(300, 3, 0, 1, seed=274)
    pair3 = _fit(X3, S.make_losses(300, seed=275), vt3, device)
    assert not (pair3.bad.variant >> 6) & 1
    C3 = S.make_candidates(900, 3, 0, 1, seed=276)
    on, st, off = _both(pair3, C3, monkeypatch, device, expect_staged=False)
    assert on.index == _oracle_pick(pair3, vt3, C3)[0]


def _random_case(seed):
    rs = np.random.RandomState(9000 + seed)
    dc = int(rs.choice([8, 16, 24, 32]))
    du = int(rs.choice([0, 4, 8]))
    D = dc + du
    n = int(rs.randint(max(40, D + 8), 601))
    nc = int(rs.choice([1, 31, 513, int(rs.randint(1, 5001))]))
    levels = rs.randint(2, 5, size=du)
    X = np.empty((n, D))
    X[:, :dc] = rs.rand(n, dc)
    if rs.rand() < 0.3:
        X[:, rs.randint(dc)] = 0.5 + 0.02 * rs.randn(n)  # a clustered column
    for u in range(du):
        X[:, dc + u] = rs.randint(0, levels[u], size=n)
    C = np.empty((nc, D))
    C[:, :dc] = rs.rand(nc, dc)
    for u in range(du):
        C[:, dc + u] = rs.randint(0, levels[u], size=nc)
    k = rs.rand(nc)
    src = X[rs.randint(0, n, size=nc)]
    C[k < 0.2] = src[k < 0.2]  # observation rows
    pt = (k >= 0.2) & (k < 0.45)
    C[pt, :dc] = src[pt, :dc] + 0.01 * rs.randn(int(pt.sum()), dc)
    C[pt, dc:] = src[pt, dc:]
    far = (k >= 0.45) & (k < 0.55)
    C[far, :dc] = 4.0 + rs.rand(int(far.sum()), dc)  # both pdfs underflow
    if nc > 4:
        C[nc // 2] = C[nc // 4]  # an exact tie
    return X, rs.rand(n), "c" * dc + "u" * du, C


@pytest.mark.parametrize("seed", range(24))
def test_random_shapes_staged_equals_unstaged(device, monkeypatch, seed):
    """Seeded random pairs in the style of test_gpu_fuzz.py over the 32x32 buckets -- dc in {8, 16, 24, 32}, du
    in {0, 4, 8}, 40-600 observations, 1-5000 candidates with observation rows, perturbed rows, far rows and a
    duplicate among them: the staged record equals the unstaged one and the pick is the oracle's."""
    X, losses, vt, C = _random_case(seed)
    if O.bohb_split(X, losses, X.shape[1] + 1) is None:
        pytest.fail("the shapes above always give a model")
    pair = _fit(X, losses, vt, device)
    supported = all((k.variant >> 7) & 1 for k in (pair.good, pair.bad))  # both on the coarse 32x32 instance
    on, st, off = _both(pair, C, monkeypatch, device, expect_staged=supported)
    assert on.index == _oracle_pick(pair, vt, C)[0], seed
