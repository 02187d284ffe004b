"""Grouped acquisition by log ratio (hbx_kde_acquire_groups_batch_lr, hbx_kde_propose_groups_lr) on the GPU against a
reference built here from the oracle's pdfs (c_oracle.kde_pdf(exact=True): pdf_many in the reference's arithmetic, the
form test_gpu_groups.py compares bit for bit) and log_pdf_many: per KDE L = log(p) for a positive normal pdf, NaN for a
negative or NaN one, the oracle's log-space value where p underflowed in a KDE without a negative match factor and
log(p) as it is otherwise; s = L_g - L_l in fp64; the winner by (s, index) with +inf last and NaN never.

Shapes (S, C): (1, 5) one partial tile; (1, 130) the chunk-splitting screen over three tiles; (3, 64) three tiles per
group -- GRP_TILES_MIN (hbx_groups.hip) is 3, so the tile screen --; (3, 70) four tiles that straddle the requests."""
import numpy as np
import pytest

from oracle import kde_oracle as O

pytestmark = pytest.mark.gpu

NEAR_TIE, OVERFLOW, NO_MODEL, SKIPPED, LOG_RATIO = 2, 1, 16, 64, 128
SHAPES = [(1, 5), (1, 130), (3, 64), (3, 70)]
#        dc, du, levels, rows of groups 0 and 2 (group 1 has D rows: no model, bohb.py:234-237)
KINDS = {"d1": (1, 0, 0, 40), "c8": (8, 0, 0, 60), "c3u2": (3, 2, 3, 120), "signed": (24, 8, 4, 240), "under": (3, 2, 3, 120),
         "cancel": (1, 1, 12, 40)}  # (test_a_g_that_may_be_negative...: 34 bad rows over 12 levels, h_u > 1)
MAIN = sorted(set(KINDS) - {"cancel"})
TINY = np.finfo(np.float64).tiny
_MODELS = {}


def _model(device, kind):
    """B = 3: group 1 without a model; c3u2 / under: group 2's last categorical column is constant (a single observed
    level: exact-only); under: the continuous columns are clustered within 1e-3, so the bandwidths are tiny"""
    from hpbandster_amd import groups
    if kind not in _MODELS:
        dc, du, nl, n = KINDS[kind]
        rs = np.random.RandomState(len(kind) + dc)
        seg = np.concatenate([[0], np.cumsum([n, dc + du, n])]).astype(np.int64)
        cont = rs.rand(seg[-1], dc) if kind != "under" else 0.5 + 1e-3 * rs.randn(seg[-1], dc)
        X = np.concatenate((cont, rs.randint(0, max(nl, 1), size=(seg[-1], du)).astype(np.float64)), axis=1)
        if kind in ("c3u2", "under"):
            X[seg[2]:, -1] = 1.0
        vt = "c" * dc + "u" * du
        gm = groups.fit_groups(X, rs.rand(seg[-1]), seg, vt, device=device)
        np.testing.assert_array_equal(gm.has_model, [True, False, True])
        hu = gm.bandwidths()[0][0, dc:]
        assert kind != "signed" or np.any(hu > 1.0)  # few good rows: the good KDE is signed
        assert kind != "c3u2" or np.all(gm.bandwidths()[1][0, dc:] < 1.0) and np.all(hu < 1.0)
        _MODELS[kind] = (gm, X, seg, vt, [0] * dc + [nl] * du)
    return _MODELS[kind]


def _reference(gm, X, seg, vt, b, x):
    """per candidate of x [C, D]: s_ref, the tolerance of s, both oracle pdfs"""
    from oracle import c_oracle
    out = []
    for kd, (rows, bw, nlev) in enumerate(zip(gm.rows_of(b), gm.bandwidths(), (gm.nlev_good, gm.nlev_bad))):
        data, bw, nlev = X[seg[b]:seg[b + 1]][rows], bw[b], nlev.cpu().numpy()[b]
        cont = np.array([c == "c" for c in vt])
        with np.errstate(all="ignore"):
            p = c_oracle.kde_pdf(data, bw, vt, nlev, x, exact=True)
            L = np.where((p != p) | (p < 0), np.nan, np.log(p))
            under = (p >= 0) & (p < TINY) & ~np.any(bw[~cont] > 1.0)
            L[under] = O.log_pdf_many(data, bw, vt, x, nlev)[under]
            # hbx_groups_lr.hip's bound of the log-space value, (D + 2) 2^-53 max|t| + (n + 256) 2^-52, with the pairs'
            # t from the fitted bandwidths: -d^2 / (2 h^2) per continuous dim, ln of the match factor per categorical one
            hu, cu = bw[~cont], np.asarray(nlev)[~cont]
            lm, ln_ = np.log(np.abs(1 - hu)), np.log(hu / (cu - 1))
            t = [-np.sum((data[:, cont] - xi[cont]) ** 2 / (2 * bw[cont] ** 2), axis=1) +
                 np.sum(np.where(data[:, ~cont] == xi[~cont], lm, ln_), axis=1) for xi in x]
            tmax = np.array([np.max(np.abs(ti[np.isfinite(ti)]), initial=0.0) for ti in t])
        ls = np.where(under, 4 * ((len(vt) + 2) * 2.0 ** -53 * tmax + (len(data) + 256) * 2.0 ** -52), 0.0)
        out.append((p, L, ls, under))
    (pl, Ll, el, ul), (pg, Lg, eg, ug) = out
    # the score's tolerance: 8 2^-53 max(1, |L_l|, |L_g|) on the exact route (two logs of at most 1 ulp and a
    # subtraction), and four times the log-space bound of each L that took that route
    mag = np.maximum(np.nan_to_num(np.abs(Ll), nan=0.0, posinf=1.0), np.nan_to_num(np.abs(Lg), nan=0.0, posinf=1.0))
    with np.errstate(all="ignore"):
        return Lg - Ll, 8 * 2.0 ** -53 * np.maximum(1.0, mag) + el + eg, pl, pg, ul | ug


def _winner(s):
    ok = np.flatnonzero(~np.isnan(s))
    return int(ok[np.argmin(s[ok])]) if len(ok) else -1


def _pools(kind, gm, rs, S, C, levels):
    dc = levels.count(0)
    pool = np.concatenate((rs.rand(gm.B, S, C, dc), rs.randint(0, max(levels[-1], 1), size=(gm.B, S, C, gm.D - dc))), axis=3)
    if kind == "under":  # near the cluster, except request (0, 0): every candidate far away, at its own distance
        pool[..., :dc] = 0.5 + 2e-3 * rs.randn(gm.B, S, C, dc)
        dist = rs.uniform(0.15, 0.4, size=(C, 1))
        dist[0] = 0.1  # (the farthest candidate has the smallest s: never index 0)
        pool[0, 0, :, :dc] = 0.5 + dist * np.sign(rs.randn(C, dc))
    pool[:, :, 1, 0] = np.nan  # a NaN coordinate is never picked
    if S > 1:
        pool[2, S - 1] = np.nan  # a request without any score
    return pool


@pytest.mark.parametrize("S,C", SHAPES)
@pytest.mark.parametrize("kind", MAIN)
def test_pick_equals_the_reference(device, kind, S, C):
    import torch
    from hpbandster_amd import groups
    gm, X, seg, vt, levels = _model(device, kind)
    rs = np.random.RandomState(1000 * S + C)
    pool = _pools(kind, gm, rs, S, C, levels)
    ref = {}
    for b in (0, 2):
        for s in range(S):
            win = _winner(_reference(gm, X, seg, vt, b, pool[b, s])[0])
            if kind == "under" and (b, s) == (0, 0) and win == 0:  # the underflow case's winner is not the lowest index
                pool[b, s, [0, 2]], win = pool[b, s, [2, 0]], 2
            if 0 <= win < C - 1:
                pool[b, s, C - 1] = pool[b, s, win]  # a bit-identical copy of the winner at a later index
            ref[b, s] = _reference(gm, X, seg, vt, b, pool[b, s])
    pd = torch.from_numpy(pool).to(device)
    raw = gm.acquire_requests(pd, sync=False, score="log_ratio").cpu().numpy()
    assert raw.tobytes() == gm.acquire_requests(pd, sync=False, score="log_ratio").cpu().numpy().tobytes()  # two runs
    rec = np.frombuffer(raw.tobytes(), dtype=groups.RECORD).reshape(gm.B, S)
    assert np.all(rec["flags"][1] == (NO_MODEL | LOG_RATIO)) and np.all(rec["index"][1] == -1)
    for (b, s), (sr, tol, pl, pg, under) in ref.items():
        r, tag, win = rec[b, s], (kind, S, C, b, s), _winner(sr)
        print(tag, "index", r["index"], "ref", win, "score", r["score"], "shortlist", r["shortlist"], "near", r["near"])
        assert r["flags"] & LOG_RATIO and not r["flags"] & (NO_MODEL | SKIPPED), tag
        assert bool(r["flags"] & OVERFLOW) == (kind in ("c3u2", "under") and b == 2), tag
        if win < 0:  # the all-NaN request (or, signed: every l of a short pool negative)
            assert r["index"] == -1 and np.isnan(r["score"]) and (kind == "signed" or (b, s) == (2, S - 1)), tag
            continue
        i = int(r["index"])
        assert i != 1 and 0 <= i < C, tag
        assert r["pdf_l"].tobytes() == pl[i].tobytes() and r["pdf_g"].tobytes() == pg[i].tobytes(), tag
        assert r["score"] == sr[i] or abs(r["score"] - sr[i]) <= tol[i], (tag, r["score"], sr[i], tol[i])
        others = np.delete(sr, [win, C - 1] if win < C - 1 else [win])  # the runner-up, the planted copy aside
        others = others[~np.isnan(others)]
        if len(others) == 0 or np.min(others) - sr[win] > tol[win]:
            assert i == win, tag
        else:
            assert (sr[i] == sr[win] or sr[i] - sr[win] <= tol[i]) and r["flags"] & NEAR_TIE, tag
        if win < C - 1:  # the planted copy ties exactly: the earlier index wins, and both are near
            assert i != C - 1 and r["near"] >= 2 and r["flags"] & NEAR_TIE, tag
        if kind == "c8":  # the screen screens: the fp32 bound is orders below the spread of s over the pool
            assert r["shortlist"] < C and (C < 64 or np.nanmax(sr) - np.nanmin(sr) > 1.0), (tag, r["shortlist"])
        if kind == "under" and (b, s) == (0, 0):  # every exact g is 0: the log-space argmin, not the lowest index
            assert np.all(pg[[0] + list(range(2, C))] == 0.0) and under[i] and win != 0 and i == win, tag
    # the all-NaN request: a prior row under NO_SCORE.  get_config draws its own pools, so a planted pool reaches its
    # finish step through finish() over the log-ratio records -- the launch get_config ends in
    if S > 1:
        fin = gm.finish(pd, gm.acquire_requests(pd, sync=False, score="log_ratio"), None, levels, 0.0, 3, 0)
        assert fin.source[2, S - 1] == groups.SOURCE_NO_SCORE and np.all(np.isfinite(fin.rows[2, S - 1]))
        assert fin.source[0, 0] == groups.SOURCE_MODEL and fin.rows[0, 0].tobytes() == pool[0, 0, rec["index"][0, 0]].tobytes()


@pytest.mark.parametrize("S,C", [(3, 64), (3, 70)])
def test_mask_and_skip_random(device, S, C):
    from hpbandster_amd import groups
    gm, X, seg, vt, levels = _model(device, "c3u2")
    pool, _ = gm.sample(C, 5, levels, requests=S)
    dense = gm.acquire_requests(pool, sync=False, score="log_ratio").cpu().numpy().reshape(gm.B * S, -1)
    m = np.array([[1, 0, 1], [0, 1, 0], [0, 0, 1]], dtype=np.uint8)
    got = gm.acquire_requests(pool, sync=False, score="log_ratio", want=m).cpu().numpy().reshape(gm.B * S, -1)
    on = m.reshape(-1) != 0
    assert got[on].tobytes() == dense[on].tobytes()
    off = np.frombuffer(got[~on].tobytes(), dtype=groups.RECORD)
    assert np.all(off["flags"] & SKIPPED) and not np.any(off["flags"] & LOG_RATIO) and np.all(off["index"] == -1)
    empty = np.frombuffer(gm.acquire_requests(pool[:, :, :0], sync=False, score="log_ratio", want=m).cpu().numpy().tobytes(),
                          dtype=groups.RECORD)  # C == 0: empty records, answered ones flagged like every other
    np.testing.assert_array_equal(empty["flags"], np.where(on, LOG_RATIO, SKIPPED))
    a = gm.get_config(C, 5, levels, requests=S, score="log_ratio")
    b = gm.get_config(C, 5, levels, requests=S, score="log_ratio", skip_random=True)
    assert a.rows.tobytes() == b.rows.tobytes() and a.source.tobytes() == b.source.tobytes()
    assert np.any(a.source == groups.SOURCE_MODEL)
    skipped = (b.picks.flags & SKIPPED) != 0  # (group 1 has no model: its source is NO_MODEL either way)
    np.testing.assert_array_equal(skipped[[0, 2]], a.source[[0, 2]] == groups.SOURCE_RANDOM_FRACTION)
    assert skipped[[0, 2]].any()


def test_a_g_that_may_be_negative_does_not_lower_the_bound(device):
    """A bad KDE with a categorical bandwidth > 1 and a planted candidate at a root of g, found by bisection on the
    oracle's pdf and taken on the side where g < 0 while l > 0: its s is NaN, its fp32 interval of g straddles 0, and
    the upper end of that interval must not prune the pool's true winner."""
    from oracle import c_oracle
    from hpbandster_amd import groups
    gm, X, seg, vt, levels = _model(device, "cancel")
    C, rs = 64, np.random.RandomState(7)
    pool = np.concatenate((rs.rand(gm.B, 1, C, 1), rs.randint(0, 12, size=(gm.B, 1, C, 1))), axis=3).astype(np.float64)
    pdf = [lambda x, kd=kd: c_oracle.kde_pdf(X[seg[0]:seg[1]][gm.rows_of(0)[kd]], gm.bandwidths()[kd][0], vt,
                                             (gm.nlev_good, gm.nlev_bad)[kd].cpu().numpy()[0], np.atleast_2d(x), exact=True)
           for kd in (0, 1)]
    assert gm.bandwidths()[1][0, 1] > 1.0
    grid, planted = np.linspace(0.0, 1.0, 201), None
    for v in range(12):
        gv = pdf[1](np.stack((grid, np.full(len(grid), float(v))), axis=1))
        for k in np.flatnonzero(gv[:-1] * gv[1:] < 0):
            neg, pos = (grid[k], grid[k + 1]) if gv[k] < 0 else (grid[k + 1], grid[k])
            for _ in range(80):
                mid = 0.5 * (neg + pos)
                neg, pos = (mid, pos) if pdf[1]([mid, v])[0] < 0 else (neg, mid)
            if planted is None and pdf[0]([neg, v])[0] > 0:
                planted = [neg, float(v)]
    assert planted is not None
    pool[0, 0, 3] = planted
    sr, tol, pl, pg, _ = _reference(gm, X, seg, vt, 0, pool[0, 0])
    win = _winner(sr)
    assert pg[3] < 0 and abs(pg[3]) < 1e-9 * np.max(np.abs(pg)) and pl[3] > 0 and np.isnan(sr[3]) and win >= 0
    assert np.min(np.delete(sr, win)[~np.isnan(np.delete(sr, win))]) - sr[win] > tol[win]
    rec = np.frombuffer(gm.acquire_requests(pool, sync=False, score="log_ratio").cpu().numpy().tobytes(), dtype=groups.RECORD)
    print("planted g", pg[3], "index", rec["index"][0], "ref", win, "shortlist", rec["shortlist"][0])
    assert rec["index"][0] == win and rec["pdf_g"][0].tobytes() == pg[win].tobytes()


def test_bohb_no_longer_returns_the_first_sample(device):
    """24c + 8u: nearly every candidate's floored score is 1, so score="ratio" picks index 0 everywhere"""
    from hpbandster_amd import groups
    gm, X, seg, vt, levels = _model(device, "signed")
    n, B = 240, 2
    idx = {}
    for score in groups.SCORES:
        opt = groups.GroupBOHB(B, vt, levels, seed=9, device=device, score=score)
        rs = np.random.RandomState(2)
        assert opt.new_results(1.0, X[:B * n].reshape(B, n, -1), rs.rand(B, n))
        gm = opt.kde_models[1.0]
        cfg = gm.get_config(opt.num_samples, 9, levels, requests=3, keep_pools=True, score=score)
        got = opt.get_configs(1.0, S=3, counter_base=0)
        assert got.rows.tobytes() == cfg.rows.tobytes()
        mb = cfg.model_based
        assert mb.any() and np.all(((cfg.picks.flags & LOG_RATIO) != 0) == (score == "log_ratio"))
        for b, s in zip(*np.nonzero(mb)):  # the model-sourced rows are the pools' rows at the records' indices
            assert cfg.rows[b, s].tobytes() == cfg.cands[b, s, cfg.picks.index[b, s]].tobytes()
        idx[score] = cfg.picks.index[mb]
    assert np.all(idx["ratio"] == 0) and np.any(idx["log_ratio"] != 0)
